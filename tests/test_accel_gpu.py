"""BeamAccelSearch on the MI355X: xengAccel* against xengPlong* itself.  The contract pins trial a to what xengPlongRun (nstack = 1)
computes when fed the series read through the trial's index map, so the core test prepares z[accel_index(alpha)] on the host,
runs xengPlong* on it and compares the trial records byte for byte, at NT = 2^15 and 2^16 (the two splits 2^7 x 2^7 and 2^7 x 2^8),
both products, and once at 2^20; the output plane is the best-over-trials rule (tests/accel_ref.py) applied to those records, H0
included.  Further: an integer-valued segment with planted equal maxima across trials and bins (the tie rule), bit identity
across splits of a run over calls, after Reset, across batch sizes and beside other engines' kernels, the planted accelerated
pulse train of tests/test_accel_cpu.py, tickets and the ABI, and Source -> BeamDedisperse -> BeamAccelSearch on device rings.  The
input bytes are compared after every call (the read-only contract), the output sits between two poisoned guard bands that are
checked after every call, the state's guards at every close.  No wall-clock assertions, and no tolerance: equality with
xengPlong* is exact, and that engine's spectra are held to its own measured bar (tests/test_plong_gpu.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import BeamAccelSearch, BeamDedisperse, accel_index, period_bands  # noqa: E402
from caltech_bifrost_dsp_amd.blocks.accel_search import ACCEL_RECORD, as_records_accel  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import accel_ref  # noqa: E402
from tests.gpu_util import Xgpu, synth_voltages  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, run_blocks  # noqa: E402
from tests.plong_ref import RECORD  # noqa: E402
from tests.test_plong_gpu import PL, _sizes, chain_case, float_case  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
NT = 1 << 15


def _info():
    n, k = ctypes.c_longlong(), ctypes.c_longlong()
    ffi.call("xengAccelGetInfo", ctypes.byref(n), ctypes.byref(k))
    return n.value, k.value


def _batch():
    a, b = ctypes.c_int(), ctypes.c_int()
    ffi.call("xengAccelGetBatch", ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


class AC:
    """The xengAccel context (one per process), an input buffer and an output plane between two poisoned guard bands."""

    def __init__(self, npair, ndm, nwin, nprod, nt, nlevel, nwhite, kedge, alphas):
        self.npair, self.ndm, self.nwin, self.nprod, self.nt, self.nlevel = npair, ndm, nwin, nprod, nt, nlevel
        self.nwhite, self.kedge, self.nband = nwhite, [int(k) for k in kedge], len(kedge) - 1
        self.alphas = [float(a) for a in alphas]
        # The buffers come first, the context second.  This file is the first of the suite to touch the GPU, and the library
        # creates its streams on first use: the order of creation decides which of them share a hardware queue for the rest of
        # the process.  The poison below goes through the copy stream, so that stream is the first one and the context's beam
        # stream the second, as when tests/test_beam_slab_parts_gpu.py, the first GPU file before this one existed, opens the
        # process with its uploads.  (tests/test_xcorr_gpu.py's check of the separate map passes only in that order.)
        self.din = ffi.DeviceBuffer(nwin * npair * ndm * nprod * 4)
        self.nbytes = npair * ndm * nlevel * self.nband * 16
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.nbytes)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        ffi.call("xengAccelInitialize", 0, npair, ndm, nwin, nprod, nt, nlevel, nwhite, self.nband, (ctypes.c_int * len(kedge))(*self.kedge),
                 len(self.alphas), (ctypes.c_double * len(self.alphas))(*self.alphas))
        self.sent = None

    def enqueue(self, x, out=True):
        """One call; returns `completed`."""
        nc = x.shape[0]
        assert x.shape == (nc, self.npair, self.ndm, self.nprod)
        self.sent = np.ascontiguousarray(x, np.float32)
        self.din.upload(self.sent)
        done = ctypes.c_int(-1)
        ffi.call("xengAccelRun", self.din.ptr, nc, self.dout.ptr + GUARD if out else None, ctypes.byref(done))
        assert done.value in (0, 1)
        return done.value

    def result(self, completed):
        """After a sync: the input bytes are what was uploaded; the plane of a completing call (the poison is put back behind it),
        or None after having checked that a call which completed nothing left the poison in the output too; every byte before and
        after it must still be poison."""
        if self.sent is not None:
            assert self.din.download(np.uint8, self.sent.nbytes).tobytes() == self.sent.tobytes(), "the input was written"
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + self.nbytes:] == POISON).all(), "bytes past the output's records were written"
        if not completed:
            assert (raw[GUARD:GUARD + self.nbytes] == POISON).all(), "a call that completed no segment wrote its output"
            return None
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        return raw[GUARD:GUARD + self.nbytes].copy().view(ACCEL_RECORD).reshape(self.npair, self.ndm, self.nlevel, self.nband)

    def run(self, x):
        done = self.enqueue(x)
        ffi.call("xengAccelSync")
        return self.result(done)

    def stream(self, x, sizes):
        """Consecutive calls of the given sizes over the windows of x; the planes of the calls that completed a segment."""
        planes, n, total = [], 0, _info()[0]
        for nc in sizes:
            want = (total + nc) // self.nt > total // self.nt
            p = self.run(x[n:n + nc])
            assert (p is not None) == want
            if p is not None:
                planes.append(p)
            n += nc
            total += nc
        assert n == x.shape[0]
        return planes

    def trial_records(self, series0=0, nser=None):
        """[ntrial][nser][nlevel][nband] (with every series: [ntrial][npair][ndm][nlevel][nband])"""
        all_ = nser is None
        nser = self.npair * self.ndm - series0 if all_ else nser
        rec = np.empty((len(self.alphas), nser, self.nlevel, self.nband), RECORD)
        ffi.call("xengAccelGetTrialRecords", series0, nser, rec.ctypes.data)
        return rec.reshape(len(self.alphas), self.npair, self.ndm, self.nlevel, self.nband) if all_ and series0 == 0 else rec

    def set_mask(self, keep):
        ffi.call("xengAccelSetMask", None if keep is None else np.ascontiguousarray(keep, np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))

    def guards_intact(self):
        ok = ctypes.c_int()
        ffi.call("xengAccelCheckGuards", ctypes.byref(ok))
        return ok.value == 1

    def close(self):
        assert self.guards_intact(), "bytes outside the state were written"
        ffi.call("xengAccelDestroy")
        self.din.free()
        self.dout.free()


def plong_on_resampled(x, nt, nlevel, nwhite, kedge, alphas, keep, nwin):
    """The records xengPlong* (nstack = 1, one context for all trials, a Reset between them) writes for the segment x [nt][npair][ndm]
    [nprod] read through every trial's index map on the host: [ntrial][npair][ndm][nlevel][nband]."""
    _, npair, ndm, nprod = x.shape
    pl = PL(npair, ndm, nwin, nprod, nt, 1, nlevel, nwhite, kedge)
    pl.set_mask(keep)
    out = []
    for alpha in alphas:
        idx = accel_index(alpha, nt)
        assert idx.tobytes() == accel_ref.accel_index(alpha, nt).tobytes() and idx.min() >= 0 and idx.max() < nt
        ffi.call("xengPlongReset")
        plane, = pl.stream(x[idx], _sizes(None, nt, nwin, nwin))
        out.append(plane)
    pl.close()
    return np.stack(out)


def check_plane(plane, trec, alphas):
    exp = accel_ref.best_over_trials(trec, alphas)
    assert plane.tobytes() == exp.tobytes(), "the plane is not the best over the trial records: %r" % (
        np.argwhere((plane['k'] != exp['k']) | (plane['ia'] != exp['ia']) | (plane['H'].view(np.uint32) != exp['H'].view(np.uint32)) |
                    (plane['H0'].view(np.uint32) != exp['H0'].view(np.uint32)))[:5],)


def check_equivalence(ac, x, trec, plane, keep, nwin):
    ref = plong_on_resampled(x, ac.nt, ac.nlevel, ac.nwhite, ac.kedge, ac.alphas, keep, nwin)
    for a in range(len(ac.alphas)):
        assert trec[a].tobytes() == ref[a].tobytes(), "trial %d (alpha %g): records differ from xengPlong* on the resampled series: %r" % (
            a, ac.alphas[a], np.argwhere((trec[a]['k'] != ref[a]['k']) | (trec[a]['H'].view(np.uint32) != ref[a]['H'].view(np.uint32)))[:5])
    check_plane(plane, trec, ac.alphas)


def trials7(nt, tie):
    """0, both extremes +-0.5 / nt, the dyadic +-tie whose products alpha * n (n - nt) are exact halves with an odd integer part, -3 tie
    whose halves have an even one (tests/test_accel_cpu.py: together they tell half-even from every other rule), and an ordinary one"""
    return [0.123 / nt, -0.5 / nt, tie, 0.0, -tie, 0.5 / nt, -3 * tie]


# ---------------------------------------------------------------- 1. equivalence with xengPlong* on the resampled series
@pytest.mark.parametrize("nt,nprod", [(1 << 15, 1), (1 << 15, 4), (1 << 16, 1), (1 << 16, 4)])
def test_trial_records_equal_plong_on_the_resampled_series(nt, nprod):
    """2 pairs x 3 trial DMs, chi^2 powers with mean / sigma = 55, one dead series and one with two NaNs in neighbouring windows (a
    map steps by 0, 1 or 2 windows: it can skip one sample, never two neighbours); 7 trials: 0 (not the first), both extremes
    +-0.5 / NT, the dyadic +-2^-21 and -3 * 2^-21 (alpha n (n - NT) is an exact half at n = 1024 * odd: half-even rounding), an ordinary one;
    5 levels, 7 bands, B = 64, a mask across a block edge; calls of random sizes and 11 windows past the segment.  Every trial's
    records equal xengPlong*'s on z[accel_index(alpha)] byte for byte; the plane is the best over them, H0 from trial 3."""
    npair, ndm, nlevel, nwhite, nwin = 2, 3, 5, 64, 1 << 13
    kedge = period_bands(nt, 7, 2)
    alphas = trials7(nt, 2.0 ** -21)
    half = alphas[2] * (1024.0 * 3) * (1024.0 * 3 - nt)
    assert half == np.floor(half) + 0.5                         # (the tie is really there)
    rng = np.random.default_rng(nt + nprod)
    x = float_case(rng, nt + 11, npair, ndm, nprod)
    x[:, 0, 1, :] = 0.0
    x[nt // 3:nt // 3 + 2, 1, 2, :] = np.nan
    keep = np.ones(nt // 2, np.uint8)
    keep[3 * nwhite - 3:3 * nwhite + 2] = 0
    ac = AC(npair, ndm, nwin, nprod, nt, nlevel, nwhite, kedge, alphas)
    ac.set_mask(keep)
    plane, = ac.stream(x, _sizes(rng, x.shape[0], nwin))
    assert _info() == (nt + 11, 1)
    trec = ac.trial_records()
    part = ac.trial_records(2, 3)                               # (a range of the series)
    assert part.tobytes() == np.ascontiguousarray(trec.reshape(len(alphas), npair * ndm, nlevel, -1)[:, 2:5]).tobytes()
    check_equivalence(ac, x[:nt], trec, plane, keep, nwin)
    ac.close()
    none = np.array([(0.0, -1, -1, 0.0)] * (nlevel * 7), ACCEL_RECORD).tobytes()
    assert plane[1, 2].tobytes() == none                        # the NaN series
    full = trec[0, 0, 0]['k'] >= 0                              # [nlevel][nband]: the bands that hold bins (the top ones are empty at high levels)
    assert full[0].all() and (full == (plane['k'] >= 0))[[0, 0, 0, 1, 1], [0, 1, 2, 0, 1]].all()
    dead = plane[0, 1]                                          # every trial ties: the first one, the band's first bin, H = h exactly
    assert (dead['ia'][full] == 0).all() and (dead['H'] == np.where(full, (1 << np.arange(nlevel))[:, None], 0)).all() and (dead['H0'] == dead['H']).all()
    for s in ((0, 0), (0, 2), (1, 0), (1, 1)):
        p = plane[s]
        assert (p['k'][full] >= 2).all() and (p['H0'][full] > 0).all() and (p['H'] >= p['H0']).all()
        assert p[~full].tobytes() == np.array([(0.0, -1, -1, 0.0)] * int((~full).sum()), ACCEL_RECORD).tobytes()
    assert len(set(plane['ia'][0, 0][full].tolist())) > 1       # (noise: the best trial varies from record to record)


def test_largest_segment_equals_plong_on_the_resampled_series():
    """NT = 2^20 (2^9 x 2^10, one row per work-group of the rows pass), 1 pair x 2 trial DMs, 3 trials: 0, +0.5 / NT and the dyadic
    -2^-31 (exact halves at n = 2^15 * odd); 3 levels, 4 bands."""
    nt, npair, ndm, nlevel, nwhite, nwin = 1 << 20, 1, 2, 3, 64, 1 << 18
    kedge = period_bands(nt, 4, 2)
    alphas = [0.0, 0.5 / nt, -2.0 ** -31]
    half = alphas[2] * (32768.0 * 3) * (32768.0 * 3 - nt)
    assert half == np.floor(half) + 0.5
    x = float_case(np.random.default_rng(20), nt, npair, ndm, 1)
    ac = AC(npair, ndm, nwin, 1, nt, nlevel, nwhite, kedge, alphas)
    plane, = ac.stream(x, [nwin] * 4)
    trec = ac.trial_records()
    check_equivalence(ac, x, trec, plane, None, nwin)
    ac.close()
    assert (plane['k'] >= 2).all() and (plane['ia'] >= 0).all()


# ---------------------------------------------------------------- 2. the tie rule
def test_integer_valued_segment_with_equal_maxima_across_trials_and_bins():
    """NT = 2^15, B = 8, every bin zapped but 40, 41, 104, 105, 3000, 3001, 9000 and 9001; each series a constant plus four tones
    of equal amplitude at 40, 104, 3000 and 9000 (tests/test_plong_gpu.py's construction with one segment): the whitened spectrum is
    1.0 everywhere and 2.0 at the tones, every harmonic sum is exact and equal maxima abound.  Trials: 1e-10 (|alpha| NT^2 / 4 <
    0.5: the identity map, but not the zero trial), 0.0, 0.0 again and -0.3 / NT, which smears the tones and can only lose.  Trials
    0, 1 and 2 give the same records bit for bit, and the rule must take ia = 0, the smallest k of the band, and H0 from trial 1."""
    npair, ndm, nt, nlevel = 2, 5, NT, 5
    kedge = [1, 64, 2000, nt // 2]
    alphas = [1e-10, 0.0, 0.0, -0.3 / nt]
    assert (accel_index(alphas[0], nt) == np.arange(nt)).all()
    n = np.arange(nt)
    amp = np.arange(1, npair * ndm + 1).reshape(npair, ndm) * 8.0
    tone = sum(np.cos(2 * np.pi * k * n / nt) for k in (40, 104, 3000, 9000))
    x = (100.0 + amp[None] * tone[:, None, None]).astype(np.float32)[..., None]
    keep = np.zeros(nt // 2, np.uint8)
    keep[[40, 41, 104, 105, 3000, 3001, 9000, 9001]] = 1
    ac = AC(npair, ndm, 8192, 1, nt, nlevel, 8, kedge, alphas)
    ac.set_mask(keep)
    plane, = ac.stream(x, [8192] * 4)
    trec = ac.trial_records()
    ac.close()
    check_plane(plane, trec, alphas)
    assert trec[0].tobytes() == trec[1].tobytes() == trec[2].tobytes()
    full = plane['k'] >= 0
    assert full[..., :4, :2].all() and full[..., :1, :].all() and not full[..., 4, 2].any()     # (16 * 2000 > N: empty)
    assert (plane['ia'][full] == 0).all() and (plane['H0'][full] == plane['H'][full]).all()
    assert (plane['H'][..., 0, :] == 2.0).all() and (plane['k'][..., 0, :] == [40, 104, 3000]).all()
    assert (plane['H'][..., 1, :] == 3.0).all() and (plane['k'][..., 1, :] == [40, 207, 5999]).all()
    assert (trec[3]['H'][..., 0, :] <= 2.0).all()


# ---------------------------------------------------------------- 3. bit identity
@pytest.mark.parametrize("nprod", [1, 4])
def test_bit_identical_across_splits_reset_batches_and_concurrent_kernels(nprod):
    """NT + 17 windows at NT = 2^15, 3 x 5 series, 3 trials: even calls, a run with stretches of single windows on either side of
    the segment boundary, a random split and calls of 5000; each follows a Reset (the second after 5000 windows of another
    series' partial segment), with batches of all 15, 1, 4 and 7 series; all give the same trial records and the same plane bit
    for bit; so does a fresh context run while X-engine contractions and xengBeamformRun are in flight."""
    npair, ndm, nwin, nt, nlevel, nwhite = 3, 5, 8192, NT, 5, 64
    kedge = period_bands(nt, 7, 2)
    alphas = [-0.31 / nt, 0.0, 0.5 / nt]
    total = nt + 17
    rng = np.random.default_rng(70 + nprod)
    x = float_case(rng, total, npair, ndm, nprod)
    ones = [8192] * 3 + [8192 - 20] + [1] * 20 + [1] * 17
    assert sum(ones) == total
    splits = [_sizes(None, total, nwin, nwin), ones, _sizes(rng, total, nwin), _sizes(None, total, 5000, 5000)]
    ac = AC(npair, ndm, nwin, nprod, nt, nlevel, nwhite, kedge, alphas)
    assert _batch() == (15, 15)
    outs = []
    for i, sizes in enumerate(splits):
        if i == 1:
            assert ac.stream(100 + x[:5000][::-1], [5000]) == []
        sb = (0, 1, 4, 7)[i]
        ffi.call("xengAccelSetBatch", sb)
        assert _batch() == (sb or 15, 15)
        ffi.call("xengAccelReset")
        assert _info() == (0, 0)
        plane, = ac.stream(x, sizes)
        assert _info() == (total, 1)
        outs.append((plane.tobytes(), ac.trial_records().tobytes()))
    check_plane(plane, ac.trial_records(), alphas)
    with pytest.raises(ffi.XengError):
        ffi.call("xengAccelSetBatch", 16)
    ac.close()
    # a fresh context beside other work: contractions on their own stream, the beamformer on this one
    nstand, bchan, btime, nbeam = 96, 8, 96, 4
    xv = synth_voltages(4 * 480, 96, 352, "full").reshape(-1)
    xg = Xgpu(352, 96, 480, max_gulps=4)
    bv = synth_voltages(btime, bchan, nstand, seed=5)
    bw = (rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand)) + 1j * rng.uniform(-1, 1, (bchan, nbeam, 2 * nstand))).astype(np.complex64)
    ffi.call("xengBeamformInitialize", 0, 2 * nstand, bchan, btime, nbeam, 0)
    bin_, bwt, bout = ffi.DeviceBuffer(bv.size).upload(bv), ffi.DeviceBuffer(bw.nbytes).upload(bw), ffi.DeviceBuffer(bchan * nbeam * btime * 8)
    ac = AC(npair, ndm, nwin, nprod, nt, nlevel, nwhite, kedge, alphas)
    try:
        xg.inbuf = ffi.DeviceBuffer(xv.size).upload(xv)
        planes, n = [], 0
        for nc in splits[0]:
            for g in range(4):
                ffi.call("xengXgpuKernelAsync", xg.inbuf.ptr + g * xg.gulp_bytes, xg.out.ptr, int(g == 3))
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            done = ac.enqueue(x[n:n + nc])
            ffi.call("xengBeamformRun", bin_.ptr, bout.ptr, bwt.ptr)
            ffi.call("xengAccelSync")
            p = ac.result(done)
            if p is not None:
                planes.append(p)
            n += nc
        ffi.call("xengXgpuSync")
        plane, = planes
        outs.append((plane.tobytes(), ac.trial_records().tobytes()))
    finally:
        xg.close()
    ac.close()
    ffi.call("xengBeamformDestroy")
    for o in outs[1:]:
        assert o[0] == outs[0][0] and o[1] == outs[0][1]


# ---------------------------------------------------------------- 4. the planted accelerated pulse train
@pytest.mark.parametrize("shift", [24, -12])
def test_planted_accelerated_pulse_train_is_found_in_its_trial(shift):
    """tests/accel_ref.planted_case (the condition on the input is checked on the restatement in tests/test_accel_cpu.py): the
    device's trial and bin per level are the float32 restatement's, the planted trial, and H >= 2 H0 (the floor under the 2.8 the
    restatement shows on the CPU)."""
    nt, nlevel, nwhite, kedge = NT, 5, 64, [2, NT // 2]
    z, alphas, planted = accel_ref.planted_case(shift)
    ref = accel_ref.best_over_trials(accel_ref.trial_records(z, nt, nlevel, nwhite, kedge, alphas), alphas)
    ac = AC(1, 1, 8192, 1, nt, nlevel, nwhite, kedge, alphas)
    plane, = ac.stream(z.reshape(nt, 1, 1, 1), [8192] * 4)
    check_plane(plane, ac.trial_records(), alphas)
    ac.close()
    got = plane[0, 0, :, 0]
    print("accel planted shift=%d: ia %s k %s H/H0 %s (restatement ia %s k %s)" % (shift, got['ia'], got['k'], got['H'] / got['H0'], ref[0, :, 0]['ia'],
                                                                                    ref[0, :, 0]['k']))
    assert (got['ia'] == planted).all() and (got['ia'] == ref[0, :, 0]['ia']).all() and (got['k'] == ref[0, :, 0]['k']).all()
    assert (got['H'] >= 2.0 * got['H0']).all() and (got['H0'] > 0).all()


# ---------------------------------------------------------------- 5. the ABI
def test_completing_call_tickets_and_argument_checks():
    """NT = 2^15, calls of 8192 windows: `completed` is 1 on the call that brings window NT and 0 on every other, whose output (NULL
    or not) is untouched.  The completing call with out_dev NULL is INVALID_ARGUMENT and enqueues nothing.  Tickets count from 1;
    unknown tickets are errors; every INVALID_ARGUMENT of Initialize leaves a live context alone; Run refuses nwin_call outside
    1..nwin and misaligned or null pointers with the count unchanged; GetTrialRecords a range outside the series and, before a
    segment has completed, INVALID_STATE; after Destroy every call that needs a context is INVALID_STATE.  The backend's accel_*."""
    npair, ndm, nt, nlevel, kedge = 2, 5, NT, 2, [2, 300, NT // 2]
    alphas = [0.0, 0.25 / nt]
    x = float_case(np.random.default_rng(3), 2 * nt, npair, ndm, 1)
    ac = AC(npair, ndm, 8192, 1, nt, nlevel, 64, kedge, alphas)
    buf = np.empty((2, npair * ndm, nlevel, 2), RECORD)
    with pytest.raises(ffi.XengError) as ei:
        ac.trial_records()
    assert ei.value.status == INVALID_STATE
    t, done = ctypes.c_ulonglong(), ctypes.c_int(-1)
    for k in range(3):
        assert ac.enqueue(x[8192 * k:8192 * k + 8192], out=k % 2 == 0) == 0
        ffi.call("xengAccelMark", ctypes.byref(t))
        assert t.value == k + 1
        ffi.call("xengAccelTicketDone", t.value, ctypes.byref(done))
        assert done.value in (0, 1)
        ffi.call("xengAccelWait", t.value)
        ffi.call("xengAccelTicketDone", t.value, ctypes.byref(done))
        assert done.value == 1 and ac.result(0) is None
    assert _info() == (3 * 8192, 0)
    with pytest.raises(ffi.XengError) as ei:
        ac.enqueue(x[3 * 8192:4 * 8192], out=False)
    assert ei.value.status == INVALID_ARGUMENT and _info() == (3 * 8192, 0)
    ffi.call("xengAccelSync")
    assert ac.result(0) is None
    plane = ac.run(x[3 * 8192:4 * 8192])
    assert plane is not None and _info() == (nt, 1)
    trec = ac.trial_records()
    check_plane(plane, trec, alphas)
    for bad in (0, 5):
        with pytest.raises(ffi.XengError):
            ffi.call("xengAccelTicketDone", bad, ctypes.byref(done))
        with pytest.raises(ffi.XengError):
            ffi.call("xengAccelWait", bad)
    from caltech_bifrost_dsp_amd.backend import HipBackend
    be = HipBackend()
    tk = be.accel_mark()
    assert tk == 4
    be.accel_wait(tk)
    be.accel_wait(tk)
    assert be.accel_ticket_done(tk) and be.accel_info() == (nt, 1) and be.accel_guards_intact() and be.accel_get_batch() == (10, 10)
    assert be.accel_trial_records(0, npair * ndm, 2, nlevel, 2).tobytes() == trec.tobytes()
    assert be.accel_set_mask(np.ones(nt // 2, np.uint8)) == 0 and be.accel_set_mask(None) == 0
    be.accel_set_batch(3)
    assert be.accel_get_batch() == (3, 10)
    be.accel_reset()
    assert be.accel_info() == (0, 0)
    with pytest.raises(ffi.XengError) as ei:
        ac.trial_records()
    assert ei.value.status == INVALID_STATE                     # (a Reset forgets the last segment)
    again, = ac.stream(x[:nt], [8192] * 4)
    assert again.tobytes() == plane.tobytes()
    second, = ac.stream(x[nt:], [8192] * 4)                     # the next segment is a search of its own
    assert _info() == (2 * nt, 2) and second.tobytes() != plane.tobytes()
    # arguments, with the context
    edges, al = (ctypes.c_int * 3)(*kedge), (ctypes.c_double * 2)(*alphas)
    good = [0, npair, ndm, 8192, 1, nt, nlevel, 64, 2, edges, 2, al]
    for i, v in ((1, 0), (3, nt + 1), (4, 2), (5, 1 << 14), (5, 1 << 21), (6, 0), (6, 6), (7, 4), (7, 1 << 14), (8, 0), (8, 33), (9, None),
                 (9, (ctypes.c_int * 3)(2, 2, 9)), (9, (ctypes.c_int * 3)(2, 300, nt // 2 + 1)), (10, 0), (10, 257), (11, None),
                 (11, (ctypes.c_double * 2)(0.0, float('nan'))), (11, (ctypes.c_double * 2)(float('inf'), 0.0)),
                 (11, (ctypes.c_double * 2)(0.0, np.nextafter(0.5 / nt, 1.0))), (11, (ctypes.c_double * 2)(-0.6 / nt, 0.0))):
        args = list(good)
        args[i] = v
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengAccelInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, (i, v)
    assert _info() == (2 * nt, 2)               # (the context is still there)
    comp = ctypes.c_int(-1)
    for args in ((ac.din.ptr, 0, ac.dout.ptr), (ac.din.ptr, 8193, ac.dout.ptr), (ac.din.ptr + 4, 1, ac.dout.ptr), (ac.din.ptr, 1, ac.dout.ptr + 8),
                 (None, 1, ac.dout.ptr)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengAccelRun", *args, ctypes.byref(comp))
        assert ei.value.status == INVALID_ARGUMENT and _info() == (2 * nt, 2)
    for s0, ns in ((-1, 1), (0, 0), (0, 11), (10, 1), (9, 2)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengAccelGetTrialRecords", s0, ns, buf.ctypes.data)
        assert ei.value.status == INVALID_ARGUMENT
    din, dout = ac.din.ptr, ac.dout.ptr
    ac.close()
    s, n = ctypes.c_int(), ctypes.c_longlong()
    for name, args in (("xengAccelRun", (din, 1, dout, ctypes.byref(s))), ("xengAccelReset", ()), ("xengAccelSetMask", (None,)), ("xengAccelSetBatch", (1,)),
                       ("xengAccelGetBatch", (ctypes.byref(s), ctypes.byref(s))), ("xengAccelGetInfo", (ctypes.byref(n), ctypes.byref(n))),
                       ("xengAccelGetTrialRecords", (0, 1, buf.ctypes.data)),
                       ("xengAccelMark", (ctypes.byref(t),)), ("xengAccelWait", (1,)), ("xengAccelTicketDone", (1, ctypes.byref(s))),
                       ("xengAccelSync", ()), ("xengAccelCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name


# ---------------------------------------------------------------- 6. the chain on device rings
def test_chain_source_dedisperse_accel_search_on_device_rings():
    """Source -> BeamDedisperse -> BeamAccelSearch (tests/test_plong_gpu.py's chain case: a pulse every 27 windows in pair 1,
    dispersed at trial 5 of 8, not accelerated) with three trials: on_candidates receives the planted pair, DM and period, found
    in the zero trial (ia = 1, accel = 0, z = 0, H0 = H); the one plane of the output ring equals a direct run of xengAccelRun on
    the spans BeamDedisperse wrote, bit for bit; the header carries the trials."""
    c = chain_case()
    npair, nwin, nt, ndm, nlevel = c['npair'], c['nwin'], c['nt'], len(c['dms']), 4
    kedge = [2, 600, 1300, 2000, nt // 2]
    alphas = [-0.2 / nt, 0.0, 0.2 / nt]
    r0, r1, r2 = Ring("ub-output", space="cuda"), Ring("dd-output", space="cuda"), Ring("ac-output", space="cuda_host")
    got = []
    dd = BeamDedisperse(LOG, r0, r1, npair=npair, nchan=c['nchan'], nupchan=c['N'], nwin=nwin, dms=c['dms'], gpu=0)
    acs = BeamAccelSearch(LOG, r1, r2, npair=npair, ndm=ndm, nwin=nwin, nt=nt, alphas=alphas, nlevel=nlevel, nwhite=64, kedge=kedge, threshold=6.0,
                          on_candidates=got.extend, gpu=0)
    mid, sink = Sink(r1, nwin * npair * ndm * 4), Sink(r2, npair * ndm * nlevel * 4 * 16)
    run_blocks([dd, acs], Source(r0, [(c['hdr'], c['x'], nwin * npair * c['nfine'] * 16)]), [mid, sink])
    (dh, _, dspans), = mid.sequences
    (hd, tag, planes), = sink.sequences
    acc_len = c['W'] * c['N']
    skipped = -(-c['S'] // nwin)
    assert skipped == 1 and len(dspans) == c['nspan'] and len(planes) == 1
    assert tag == hd['seq0'] == 4096 + skipped * nwin * acc_len
    assert (hd['nt'], hd['nlevel'], hd['nwhite'], hd['nband'], hd['kedge'], hd['ntrial'], hd['alpha'], hd['dedisp_latency']) == (
        nt, nlevel, 64, 4, kedge, 3, alphas, c['S'])
    assert hd['accel'][1] == 0.0 and hd['accel'][2] == -hd['accel'][0] > 0
    best = [g for g in got if g['pair'] == 1]
    assert best and {g['pair'] for g in got} == {1}, got
    top = min(best, key=lambda g: g['log10_pfa'])
    assert abs(top['k'] / top['h'] - nt / 27) <= 0.5 and top['band'] == 1 and top['harmonics'] and top['sigma'] > 6
    assert abs(top['period'] - 27 * c['tsamp']) < 1e-3 * top['period'] and abs(top['idm'] - c['d0']) <= 1
    assert (top['ia'], top['accel'], top['z']) == (1, 0.0, 0.0) and top['H0'] == top['H']
    assert acs.stats['ncand'] == len(got) and acs.stats['nstartup'] == skipped and acs.stats['nwindow'] == (c['nspan'] - skipped) * nwin
    assert acs.stats['nstack_done'] == 1 and acs.stats['ndropped'] == 0
    direct = AC(npair, ndm, nwin, 1, nt, nlevel, 64, kedge, alphas)
    out = direct.stream(np.concatenate([sp.view(np.float32).reshape(nwin, npair, ndm, 1) for sp in dspans[skipped:]]), [nwin] * (c['nspan'] - skipped))
    direct.close()
    assert len(out) == 1 and out[0].tobytes() == planes[0].tobytes()
    assert (as_records_accel(planes[0], npair, ndm, nlevel, 4)['ia'][:, :, 0] >= 0).all()
