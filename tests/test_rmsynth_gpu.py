"""BeamRmSynth on the MI355X: xengRmsynth* against the restatement (tests/rmsynth_ref.py), byte for byte and with no tolerance --
the records, the Faraday spectrum, the de-rotated profile and the poison around them; which words are NaN is compared, a NaN's sign
and payload are not (the contract leaves them open).  The output sits between poisoned guard bands that are checked after every
call, the input is read back after every call and must be what was uploaded, the state's guards are checked at every close.  The
shapes are the smallest at which each mechanism can fail (the docstrings say which).  The Faraday words against the float64
statement (blocks/rm_synth.py rm_reference) within the a-priori bound; BeamFold(stokes='full') -> BeamRmSynth through rings on the
device.  No wall-clock assertions."""
import ctypes
import json
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import caltech_bifrost_dsp_amd  # noqa: E402,F401
from caltech_bifrost_dsp_amd import ffi  # noqa: E402
from caltech_bifrost_dsp_amd.blocks import BeamFold, BeamRmSynth, rm_lambda2, rm_reference, rm_table  # noqa: E402
from caltech_bifrost_dsp_amd.ring import Ring  # noqa: E402
from tests import rmsynth_cases, rmsynth_ref  # noqa: E402
from tests.pipeline_util import LOG, Sink, Source, source_header, wait_for  # noqa: E402

POISON = 0xA5
GUARD = 1 << 16
INVALID_ARGUMENT, INVALID_STATE = 1, 2
EPS = 2.0 ** -24
_pf, _pb = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)


def _info():
    n, k, a, b, c = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
    ffi.call("xengRmsynthGetInfo", ctypes.byref(n), ctypes.byref(k), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return n.value, k.value, a.value, b.value, c.value


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, np.uint8).ctypes.data_as(_pb)


class RM:
    """The xengRmsynth context (one per process), an input buffer, the output between poisoned guard bands, and what the
    restatement needs beside it: every call goes to both and is compared byte for byte."""

    def __init__(self, npair, nchg, nbin, nphi, feeds):
        self.npair, self.nchg, self.nbin, self.nphi, self.feeds = npair, nchg, nbin, nphi, feeds
        self.out_bytes = rmsynth_ref.offsets(npair, nphi, nbin)[2]
        # the buffers come first, the context second: tests/test_accel_gpu.py says why
        self.din = ffi.DeviceBuffer(npair * 4 * nchg * nbin * 4)
        self.dout = ffi.DeviceBuffer(2 * GUARD + self.out_bytes)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        ffi.call("xengRmsynthInitialize", 0, npair, nchg, nbin, nphi, feeds)
        assert _info() == (0, -1) + rmsynth_ref.offsets(npair, nphi, nbin)
        self.T = self.w = self.use = self.off = self.on = self.active = None

    def set_table(self, T, w, use):
        self.T, self.w, self.use = np.ascontiguousarray(T, np.float32), None if w is None else np.ascontiguousarray(w, np.float32), use
        ffi.call("xengRmsynthSetTable", self.T.ctypes.data_as(_pf), None if w is None else self.w.ctypes.data_as(_pf), _u8(use))
        assert _info()[1] == (self.nchg if use is None else int(np.count_nonzero(use)))

    def set_masks(self, off, on):
        self.off, self.on = off, on
        ffi.call("xengRmsynthSetMasks", _u8(off), _u8(on))

    def set_active(self, active):
        self.active = active
        ffi.call("xengRmsynthSetActive", _u8(active))

    def run(self, X, compare=True):
        """The device's output bytes (NaNs canonical) after every check; compared with the restatement unless told not to."""
        sent = np.ascontiguousarray(X, np.float32)
        self.din.upload(sent)
        ffi.call("xengRmsynthRun", self.din.ptr, self.dout.ptr + GUARD)
        ffi.call("xengRmsynthSync")
        assert self.din.download(np.uint8, sent.nbytes).tobytes() == sent.tobytes(), "the input was written"
        raw = self.dout.download(np.uint8)
        assert (raw[:GUARD] == POISON).all(), "bytes before the output were written"
        assert (raw[GUARD + self.out_bytes:] == POISON).all(), "bytes past the output were written"
        got = rmsynth_ref.canonical(raw[GUARD:GUARD + self.out_bytes], self.npair)
        ffi.call("xengMemset", self.dout.ptr, POISON, self.dout.nbytes)
        if compare:
            exp = rmsynth_ref.canonical(rmsynth_ref.out_bytes(*rmsynth_ref.rmsynth(sent, self.T, self.w, self.use, self.off, self.on, self.active, self.feeds)),
                                        self.npair)
            bad = np.flatnonzero(got != exp)
            a, b, _ = rmsynth_ref.offsets(self.npair, self.nphi, self.nbin)
            assert bad.size == 0, "the output differs from byte %d on (%d bytes; spec begins at %d, the profile at %d)" % (bad[0], bad.size, a, b)
        return got

    def split(self, got):
        return rmsynth_ref.split_out(got, self.npair, self.nphi, self.nbin)

    def close(self):
        ok = ctypes.c_int()
        ffi.call("xengRmsynthCheckGuards", ctypes.byref(ok))
        assert ok.value == 1, "bytes outside the state were written"
        ffi.call("xengRmsynthDestroy")
        self.din.free()
        self.dout.free()


def _scene(kind, seed, nbin, use):
    X = rmsynth_cases.float_scene(seed, 2, 70, nbin) if kind == 'float' else rmsynth_cases.integer_scene(seed, 2, 70, nbin, top=20)
    return rmsynth_cases.poison_left_out(X, use)


@pytest.mark.parametrize("nphi", [1, 65, 130])
@pytest.mark.parametrize("nbin", [5, 64, 100])
def test_float_and_integer_data_equal_the_restatement_byte_for_byte(nbin, nphi):
    """2 pairs x 70 groups (nine chunks of 8, the last with 4 of the 68 used; NaN and Inf in the two groups of weight 0).  nbin 5: one
    ragged tile, word-by-word loads; 64: one full tile and run, 16-byte loads; 100: a second run of 36.  nphi 1: one depth, an odd
    row of the table (word-by-word loads); 65: a second tile of one depth; 130: even rows (16-byte loads), a third tile of two.
    Both feeds; chi-squared float data under full masks, integer data under partial masks that differ per pair, a pair without
    off-pulse bins (its baseline is +0), a pair without on-pulse bins (k = -1), and pair 1 inactive (nothing read, all +0)."""
    T, w, use = rmsynth_cases.table(70, nphi)
    for feeds in (0, 1):
        rm = RM(2, 70, nbin, nphi, feeds)
        try:
            rm.set_table(T, w, use)
            for n, (kind, mk) in enumerate((('float', 'full'), ('integer', 'partial'), ('float', 'empty_off'), ('float', 'empty_on'))):
                off, on = rmsynth_cases.masks(mk, 2, nbin)
                rm.set_masks(off, on)
                rec, spec, prof = rm.split(rm.run(_scene(kind, 10 * nbin + nphi + n, nbin, use)))
                assert np.isfinite(spec).all() and np.isfinite(prof).all() and rec['n_on'].tolist() == on.sum(1).tolist()
                assert rec['n_off'].tolist() == off.sum(1).tolist() and (rec['k'] >= 0).tolist() == [mk != 'empty_on', True]
                if mk == 'empty_on':
                    assert not spec[0].any() and not prof[0, 1:3].any() and prof[0, 0].any()
            rm.set_masks(*rmsynth_cases.masks('partial', 2, nbin))
            rm.set_active(np.array([1, 0], np.uint8))
            rec, spec, prof = rm.split(rm.run(_scene('float', 7, nbin, use)))
            assert rec[1].tolist() == (-1, 0.0, 0, 0) and not spec[1].any() and not prof[1].any() and rec[0]['k'] >= 0 and spec[0].any()
            assert _info()[0] == 5
        finally:
            rm.close()


def test_heavy_ties_and_a_nan_in_a_used_channel():
    """Constant data: y = 0 everywhere, every word of spec +0, the tie goes to k = 0 with peak +0.  One NaN in a used channel at
    an on-pulse bin of pair 0: that bin's Faraday words are NaN at every depth, so is spec, nothing is comparable (k = -1), and of
    the profile only that bin's words; one NaN at an off-pulse bin of pair 1: the baseline of that channel is NaN, every bin's
    words with it.  Then the first NaN in a bin that no mask holds: it stays in its bin's profile words and the spectrum is finite.
    A NaN is never picked; all equal the restatement (RM.run compares)."""
    T, w, use = rmsynth_cases.table(70, 130)
    off, on = rmsynth_cases.masks('partial', 2, 100)
    rm = RM(2, 70, 100, 130, 0)
    try:
        rm.set_table(T, w, use)
        rm.set_masks(off, on)
        rec, spec, prof = rm.split(rm.run(np.full((2, 4, 70, 100), 2.5, np.float32)))
        assert rec['k'].tolist() == [0, 0] and rec['peak'].tolist() == [0, 0] and not spec.any() and not prof.any()
        X = rmsynth_cases.float_scene(9, 2, 70, 100)
        b_on, b_off = int(np.flatnonzero(on[0])[3]), int(np.flatnonzero(off[1])[40])
        X[0, 0, 5, b_on] = np.nan
        X[1, 2, 30, b_off] = np.nan
        rec, spec, prof = rm.split(rm.run(X))
        assert rec['k'].tolist() == [-1, -1] and np.isnan(spec).all()
        assert np.flatnonzero(np.isnan(prof[0, 0])).tolist() == [b_on] and not np.isnan(prof[0, 3]).any() and not prof[0, 1:3].any()
        assert np.isfinite(prof[1, 0]).all() and np.isfinite(prof[1, 3]).all()
        # the same NaN in a bin that is neither on-pulse nor off-pulse: the spectrum is finite and only that bin's I, Q and U are NaN
        on2 = on.copy()
        on2[0, b_on] = 0
        rm.set_masks(off, on2)
        X[1, 2, 30, b_off] = 0.5
        rec, spec, prof = rm.split(rm.run(X))
        assert (rec['k'] >= 0).all() and np.isfinite(spec).all() and np.isnan(prof[0, 1, b_on]) and np.isnan(prof[0]).sum() == 3
    finally:
        rm.close()


def test_a_sub_list_of_depths_a_second_call_a_reset_and_a_fresh_context_give_the_same_bytes():
    """33 of the 130 depths (every fourth from the second): spec of the short table equals those words of the full spectrum bit for
    bit -- a word of spec reads one column of the table, whatever tile it falls in.  A second call, a call after other data and a
    Reset, and a fresh context give the full call's bytes again."""
    T, w, use = rmsynth_cases.table(70, 130)
    X = rmsynth_cases.poison_left_out(rmsynth_cases.float_scene(21, 2, 70, 100), use)
    off, on = rmsynth_cases.masks('partial', 2, 100)
    pick = np.arange(1, 130, 4)
    assert pick.size == 33
    rm = RM(2, 70, 100, 130, 1)
    try:
        rm.set_table(T, w, use)
        rm.set_masks(off, on)
        first = rm.run(X)
        assert rm.run(X, compare=False).tobytes() == first.tobytes()
        rm.run(rmsynth_cases.float_scene(22, 2, 70, 100), compare=False)
        ffi.call("xengRmsynthReset")
        assert _info()[0] == 0
        assert rm.run(X, compare=False).tobytes() == first.tobytes()
    finally:
        rm.close()
    full = rmsynth_ref.split_out(first, 2, 130, 100)[1]
    rm = RM(2, 70, 100, 33, 1)
    try:
        rm.set_table(T[:, pick], w, use)
        rm.set_masks(off, on)
        sub = rm.split(rm.run(X))[1]
        assert np.array_equal(sub.view(np.uint32), full[:, pick].view(np.uint32))
    finally:
        rm.close()
    rm = RM(2, 70, 100, 130, 1)
    try:
        rm.set_table(T, w, use)
        rm.set_masks(off, on)
        assert rm.run(X, compare=False).tobytes() == first.tobytes()
    finally:
        rm.close()


def test_faraday_words_are_within_the_a_priori_bound_of_the_float64_statement():
    """Every Faraday word F[p][b][k] of 2 pairs x 100 bins x 130 depths, read off the device one depth at a time (a context of one
    depth: the profile's Q and U are that depth's words), against rm_reference in float64:
    |F - F64| <= (2 nused + 4) 2^-24 sum_g (|y_q| + |y_u|)(|Tc| + |Ts|): 2 nused roundings of the chain's fmaf steps, and 4 for the
    Stokes word, the baseline and the subtraction.  The words also equal the restatement's cube bit for bit."""
    nbin, nphi = 100, 130
    T, w, use = rmsynth_cases.table(70, nphi)
    X = rmsynth_cases.poison_left_out(rmsynth_cases.float_scene(31, 2, 70, nbin), use)
    off, on = rmsynth_cases.masks('partial', 2, nbin)
    e = rm_reference(np.where(np.isfinite(X), X, 0.0), T, w, use, off, on, None, 0)
    _, _, _, Fre, Fim = rmsynth_ref.rmsynth(X, T, w, use, off, on, None, 0, cube=True)
    got = np.zeros((2, nbin, nphi), np.complex128)
    rm = RM(2, 70, nbin, 1, 0)
    try:
        rm.set_masks(off, on)
        for k in range(nphi):
            rm.set_table(np.ascontiguousarray(T[:, k:k + 1]), w, use)
            rec, _, prof = rm.split(rm.run(X, compare=False))
            assert rec['k'].tolist() == [0, 0]
            assert np.array_equal(prof[:, 1].view(np.uint32), Fre[:, :, k].view(np.uint32)) and np.array_equal(prof[:, 2].view(np.uint32), Fim[:, :, k].view(np.uint32))
            got[:, :, k] = prof[:, 1].astype(np.float64) + 1j * prof[:, 2].astype(np.float64)
    finally:
        rm.close()
    bound = (2 * e['nused'] + 4) * EPS * e['scale']
    err = np.maximum(np.abs(got.real - e['F'].real), np.abs(got.imag - e['F'].imag))
    print("rmsynth: worst |F - F64| / bound = %.3g over %d words" % ((err / bound).max(), err.size))
    assert e['nused'] == 68 and (bound > 0).all() and (err <= bound).all()


def test_refusals():
    L = ffi.lib()
    L.xengRmsynthDestroy()
    assert L.xengRmsynthInitialize(0, 2, 8, 16, 4, 0) == 0
    try:
        buf = ffi.DeviceBuffer(1 << 16)
        assert L.xengRmsynthRun(buf.ptr, buf.ptr + 32768) == INVALID_STATE                 # (no table yet)
        T = np.zeros((8, 4, 2), np.float32)
        w = np.ones(8, np.float32)
        use = np.ones(8, np.uint8)
        assert L.xengRmsynthSetTable(None, w.ctypes.data_as(_pf), _u8(use)) == INVALID_ARGUMENT
        w[3] = np.inf
        assert L.xengRmsynthSetTable(T.ctypes.data_as(_pf), w.ctypes.data_as(_pf), _u8(use)) == INVALID_ARGUMENT
        w[3] = 1
        T[5, 2, 1] = np.nan
        assert L.xengRmsynthSetTable(T.ctypes.data_as(_pf), w.ctypes.data_as(_pf), _u8(use)) == INVALID_ARGUMENT
        assert L.xengRmsynthRun(buf.ptr, buf.ptr + 32768) == INVALID_STATE                 # (a refused table is no table)
        use[5] = 0
        assert L.xengRmsynthSetTable(T.ctypes.data_as(_pf), w.ctypes.data_as(_pf), _u8(use)) == 0 and _info()[1] == 7    # (a NaN in a row left out is never read)
        for a, b in ((None, buf.ptr), (buf.ptr, None), (buf.ptr + 4, buf.ptr + 32768), (buf.ptr, buf.ptr + 32768 + 8)):
            assert L.xengRmsynthRun(a, b) == INVALID_ARGUMENT
        assert _info()[0] == 0
        ffi.call("xengMemset", buf.ptr, 0, buf.nbytes)
        assert L.xengRmsynthRun(buf.ptr, buf.ptr + 32768) == 0
        t = ctypes.c_ulonglong()
        ffi.call("xengRmsynthMark", ctypes.byref(t))
        ffi.call("xengRmsynthWait", t.value)
        done = ctypes.c_int()
        ffi.call("xengRmsynthTicketDone", t.value, ctypes.byref(done))
        assert done.value == 1 and _info()[0] == 1
        buf.free()
    finally:
        ffi.call("xengRmsynthDestroy")


# ---------------------------------------------------------------- BeamFold(stokes='full') -> BeamRmSynth through rings
@pytest.mark.parametrize("space", ["cuda", "cuda_host"])
def test_fold_then_rm_synthesis_through_rings_on_the_device(space):
    """2 pairs x 96 fine channels over 60 to 79.6 MHz, windows folded into 16 bins by a pulsar whose period is 16 windows (window n
    falls in bin n mod 16), pair 1 without a pulsar.  The power beams carry a pulse of sigma 1 bin at bin 8, 60 % linear,
    Faraday-rotated by 1.37 rad/m^2, and noise.  BeamFold(stokes='full', nfscr=1) writes one cube per 4 spans of 16 windows;
    BeamRmSynth reads that ring in device space (directly) or in pinned host space (one staged copy per span) and writes records,
    spectrum and profile.  The record's depth lies within dphi / 2 of the planted one, and the whole output equals the restatement fed
    the fold's own span with the table made from the header's frequencies."""
    npair, nchan, N, W, nwin, nbin, nsub, nspan, rm_true = 2, 3, 32, 1, 16, 16, 4, 8, 1.37
    nfine = nchan * N
    chan_bw = 19.6e6 / nchan
    hdr = source_header(nchan, npair, 2, seq0=0, sfreq=60e6, chan_bw=chan_bw)
    hdr.update(nstand=npair, nbeam=npair, npol=2, complex=True, nbit=32, nupchan=N, nframe_sum=W, fine_bw_hz=chan_bw / N, fine_sfreq=60e6, pair0=0, acc_len=W * N)
    tsamp = W * N * nchan / hdr['bw_hz']
    pulsars = [dict(f0=1.0 / (nbin * tsamp), f1=0.0, pepoch=0.0, dm=0.0), None]
    freqs = hdr['fine_sfreq'] + hdr['fine_bw_hz'] * np.arange(nfine)
    rng = np.random.default_rng(77)
    total = nspan * nwin
    b = (np.arange(total) % nbin)[:, None, None]
    I = 1.0 + 10.0 * np.exp(-0.5 * (b - 8.0) ** 2) * np.ones((1, npair, nfine))
    chi = 0.3 + rm_true * rm_lambda2(freqs)[None, None, :]
    Q, U = 0.6 * (I - 1.0) * np.cos(2 * chi), 0.6 * (I - 1.0) * np.sin(2 * chi)
    x = np.stack([(I + Q) / 2, (I - Q) / 2, U / 2, 0.05 * I], axis=-1) + 0.3 * rng.standard_normal((total, npair, nfine, 4))
    x = np.ascontiguousarray(x, np.float32)
    phis = rmsynth_cases.phis(130)
    r0, r1, r2 = Ring("rm-power", space="cuda"), Ring("rm-fold", space=space), Ring("rm-out", space="cuda_host")
    fold = BeamFold(LOG, r0, r1, npair=npair, nchan=nchan, nupchan=N, nwin=nwin, nbin=nbin, pulsars=pulsars, nsub=nsub, nfscr=1, stokes='full', gpu=0)
    rms = BeamRmSynth(LOG, r1, r2, npair=npair, nchg=nfine, nbin=nbin, phis=phis, feeds='linear', gpu=0)
    cube_bytes = npair * 4 * nfine * nbin * 4
    sinks = [Sink(r1, cube_bytes), Sink(r2, rmsynth_ref.offsets(npair, 130, nbin)[2])]
    ths = [threading.Thread(target=blk.main, daemon=True) for blk in (fold, rms)]
    for t in sinks + ths:
        t.start()
    wait_for(lambda: len(r0._readers) >= 1 and len(r1._readers) >= 2 and len(r2._readers) >= 1, "the readers")
    src = Source(r0, [(hdr, x, nwin * npair * nfine * 16)])
    src.start()
    for t in [src] + ths + sinks:
        t.join(60)
        assert not t.is_alive(), "pipeline thread did not finish: %r" % (t,)
    cubes, outs = sinks[0].sequences, sinks[1].sequences
    assert len(cubes) == len(outs) == nspan // nsub
    T, w, use, lam0 = rm_table(freqs, phis, None)
    for (ch, ctag, cspans), (oh, otag, ospans) in zip(cubes, outs):
        assert len(cspans) == len(ospans) == 1 and otag == ctag and ch['nprod'] == 4 and 'rm_phis' not in ch
        assert oh['rm_phis'] == phis.tolist() and oh['lambda0_sq'] == lam0 and oh['rm_feeds'] == 'linear' and oh['nbin'] == nbin
        a, bb, n = rmsynth_ref.offsets(npair, 130, nbin)
        assert (oh['record_offset'], oh['spec_offset'], oh['profile_offset'], oh['span_bytes']) == (0, a, bb, n)
        assert oh['rm_n_on'] == [nbin, nbin] and oh['rm_n_off'] == [nbin, nbin]
        cube = cspans[0].view(np.float32).reshape(npair, 4, nfine, nbin)
        exp = rmsynth_ref.canonical(rmsynth_ref.out_bytes(*rmsynth_ref.rmsynth(cube, T, w, use, None, None, np.array([1, 0], np.uint8), 0)), npair)
        got = rmsynth_ref.canonical(ospans[0], npair)
        assert got.tobytes() == exp.tobytes()
        rec, spec, prof = rmsynth_ref.split_out(got, npair, 130, nbin)
        assert abs(phis[rec[0]['k']] - rm_true) <= rmsynth_cases.DPHI / 2 and rec[1].tolist() == (-1, 0.0, 0, 0) and not spec[1].any()
        assert int(np.argmax(np.hypot(prof[0, 1], prof[0, 2]))) == 8
    assert rms.stats['nsubint'] == nspan // nsub and rms.stats['npeak'] == nspan // nsub
    assert json.dumps(outs[0][0])        # (the header is plain JSON)
