"""UpchanGainCal without a GPU: the restatement (tests/gaincal_ref.py) against a textbook dense StEFCal, on noise-free visibilities
(recovery of the gains, the iterations that takes, the averaging step), with a flagged stand that holds NaN; what a caller does with
a solution (blocks/calibration.py: apply_gains and the imager, inverse_gains, reference_phase, model_visibilities); the block on CPU
rings (both implementations) with a backend, defined here, that serves gaincal_* from the restatement -- header keys, one output
span per integration, the commands at the next integration, a gap, the warm and cold starts, the refusals -- and the C entry points'
argument checks."""
import ctypes
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import (UpchanGainCal, apply_gains, inverse_gains, model_flux, model_visibilities, reference_phase,
                                            steering_delays)
from caltech_bifrost_dsp_amd.ring import Ring
from tests.fake_backend import OracleBackend
from tests.gaincal_ref import corrupt, float_gap, gain_error, model, noisy, read_block, setup, sky, solve, steering, textbook_stefcal
from tests.image_ref import image, random_array
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
FINE_BW = 23925.78125 / 2
SHAPES = [(22, 1, 4), (35, 3, 3), (64, 32, 2)]  # (nstand, nsrc, nfine): a partial tile, one tile and a bit, two whole tiles
# test_noise_free_gains_are_recovered's measurements: the iterations the slowest (channel, pol) needs at tol = 1e-6
ITERATIONS = {(22, 1, 4): 14, (35, 3, 3): 30, (64, 32, 2): 28}


@pytest.fixture(params=["native", "python"])
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


def _case(nstand, nsrc, nfine):
    """Arrays of 1.2 km, gains of amplitude 0.5 to 2 and any phase, stand 3 flagged: (tau, freq, flux, w, true gains, V)"""
    rng, tau, freq, flux, w, g = setup(100 + nstand, nstand, nsrc, nfine)
    return tau, freq, flux, w, g, corrupt(model(freq, tau, flux), g)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_is_textbook_stefcal_in_float64(shape):
    """The contract's route (the contraction over the sources' steering rows, D from the Gram matrix minus the t = s term) against
    the dense iteration on model_visibilities, 20 iterations of each: measured 9.0e-16 (22 stands, 1 source), 1.1e-15 (35, 3) and
    2.2e-15 (64, 32) as max_s |g - g'| / rms |g'| -- rounding; asserted with a margin of 10 on the worst."""
    tau, freq, flux, w, g, V = _case(*shape)
    V = noisy(np.random.default_rng(1), V, 0.02)
    a = solve(V, freq, tau, flux, w, 0, 20, 0.0)[0]
    b = textbook_stefcal(V, model_visibilities(freq, tau, flux), w, 0, 20)
    err = gain_error(a, b).max()
    print("restatement against the dense iteration, %r: %.2e" % (shape, err))
    assert err <= 10 * 2.2e-15


@pytest.mark.parametrize("shape", SHAPES)
def test_noise_free_gains_are_recovered(shape):
    """V = g g^H o M (rounded to complex64), tol = 1e-6, from g = 1.  Measured on the CPU, float64 and complex64 alike:
        22 stands,  1 source : 12 to 14 iterations per (channel, pol), final error 3.0e-7 (complex64: 4.4e-7)
        35 stands,  3 sources: 18 to 30 iterations,                    final error 2.0e-6 (complex64: 2.1e-6)
        64 stands, 32 sources: 14 to 28 iterations,                    final error 2.2e-6 (complex64: 2.5e-6)
    as max_s |g - g_true| / rms |g_true| after both are phase referenced.  ITERATIONS holds the largest count of each shape; the
    GPU tests use those.  The bound on the error: consecutive iterates within delta <= 1e-6 of each other and a measured
    contraction of about a half per pair of iterations leave the fixed point within a few delta; 1e-5 is ten delta."""
    tau, freq, flux, w, g, V = _case(*shape)
    truth = reference_phase(np.where(w != 0, g, 0), 0)
    for dtype in (np.complex128, np.complex64):
        got, stats, _ = solve(V, freq, tau, flux, w, 0, ITERATIONS[shape], 1e-6, dtype)
        err = gain_error(got, truth).max()
        print("%r %s: iterations %s, error %.2e" % (shape, np.dtype(dtype).name, stats[:, :, 0].ravel(), err))
        assert (stats[:, :, 3] == 1).all() and stats[:, :, 0].max() == ITERATIONS[shape] and (stats[:, :, 2] == shape[0] - 1).all()
        assert err <= 1e-5 and (got[:, :, 3] == 0).all() and np.abs(got[:, :, 0].imag).max() <= 1e-6


@pytest.mark.parametrize("shape", SHAPES)
def test_without_the_averaging_step_the_same_case_does_not_converge(shape):
    """The plain iteration g <- N / D oscillates between two points: in the count that suffices with the average no (channel, pol)
    converges, and the gains are wrong by more than their own size."""
    tau, freq, flux, w, g, V = _case(*shape)
    got, stats, _ = solve(V, freq, tau, flux, w, 0, ITERATIONS[shape], 1e-6, average=False)
    assert (stats[:, :, 3] == 0).all() and (stats[:, :, 1] > 0.1).all()
    assert gain_error(got, reference_phase(np.where(w != 0, g, 0), 0)).min() > 0.5


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_flagged_stand_holding_nan_is_the_stand_deleted(dtype):
    """w_3 = 0 and NaN / Inf all over stand 3's rows and columns: the solution is finite, stand 3's gain is 0, and it is bit for bit
    the solution of the matrix with zeros there; the other stands' gains are those of the array without stand 3 to rounding (numpy's
    sums take another order for another length)."""
    tau, freq, flux, w, g, V = _case(12, 3, 2)
    bad, zeros = V.copy(), V.copy()
    bad[:, 3] = np.nan
    bad[:, :, :, 3] = np.inf
    zeros[:, 3] = 0
    zeros[:, :, :, 3] = 0
    got, stats, _ = solve(bad, freq, tau, flux, w, 5, 12, 0.0, dtype)
    same, sstats, _ = solve(zeros, freq, tau, flux, w, 5, 12, 0.0, dtype)
    assert np.isfinite(got).all() and (got[:, :, 3] == 0).all() and np.array_equal(got, same) and np.array_equal(stats, sstats)
    keep = np.arange(12) != 3
    exp, estats, _ = solve(V[:, keep][:, :, :, keep], freq, tau[:, keep], flux, w[keep], 4, 12, 0.0, dtype)
    assert gain_error(got[:, :, keep], exp).max() <= 100 * np.finfo(dtype).eps and np.array_equal(stats[:, :, [0, 2, 3]], estats[:, :, [0, 2, 3]])
    assert np.isfinite(read_block(bad, w, 0, 1)).all()


def test_steering_convention_is_the_imagers_and_x_is_v_of_a_hermitian_matrix():
    """a_ks is image_ref.steering's factor with unit weights; model_visibilities is a a^H summed over the sources with a real
    positive diagonal sum_k F_k; read_block of a Hermitian matrix is its pp block without the diagonal."""
    from tests.image_ref import steering as image_steering
    tau, freq, flux, w, g, V = _case(9, 3, 2)
    assert np.array_equal(steering(freq, tau), image_steering(freq, tau, np.ones(9)))
    M = model_visibilities(freq, tau, flux)
    assert M.shape == (2, 9, 9) and np.allclose(M, np.conj(M.transpose(0, 2, 1))) and np.allclose(np.einsum('css->cs', M), flux.sum(axis=1, keepdims=True))
    assert np.array_equal(model_visibilities(freq, tau, flux[0]), model_visibilities(freq, tau, np.broadcast_to(flux[0], flux.shape)))
    X = read_block(V, np.ones(9), 1, 0)
    assert np.array_equal(X, np.where(np.eye(9, dtype=bool), 0, V[1, :, 0, :, 0]))
    for bad in (dict(flux=[1.0, 2.0]), dict(flux=-flux), dict(flux=np.full((2, 3), np.nan)), dict(tau=tau[0])):
        kw = dict(freq=freq, tau=tau, flux=flux)
        kw.update(bad)
        with pytest.raises(ValueError, match="model_"):
            model_visibilities(**kw)
    assert model_flux([1, 2, 3], 2, 3).shape == (2, 3)


# ---------------------------------------------------------------- what a caller does with a solution
def test_applying_the_solution_makes_a_point_source_read_one_at_its_pixel():
    """One source of flux 1 at list pixel 5 of 9 seen through gains of amplitude 0.5 to 2: the dirty image of the raw visibilities
    does not read 1 there; after apply_gains of the solution XX and YY read 1 within 1e-5 (the solution's own error, tol = 1e-6)
    and peak there.  The flagged stand's rows and columns are zeros after apply_gains whatever they held."""
    nstand, nfine, x0 = 22, 2, 5
    rng = np.random.default_rng(5)
    pos, lmn = random_array(rng, nstand, 1200.0, 5.0), sky(rng, 9)
    tau_pix = steering_delays(pos, lmn)
    freq = 50e6 + FINE_BW * np.arange(nfine)
    w = np.ones(nstand, np.float32)
    w[3] = 0
    g = rng.uniform(0.5, 2.0, (nfine, 2, nstand)) * np.exp(2j * np.pi * rng.uniform(size=(nfine, 2, nstand)))
    V = corrupt(model_visibilities(freq, tau_pix[x0:x0 + 1], [1.0]), g)
    V[:, 3] = np.nan
    V[:, :, :, 3] = np.nan
    raw = image(V, freq, tau_pix, w, False, 1)
    got, stats, _ = solve(V, freq, tau_pix[x0:x0 + 1], [1.0], w, 0, 40, 1e-6)
    assert (stats[:, :, 3] == 1).all()
    cal = apply_gains(V, got)
    assert np.isfinite(cal).all() and (cal[:, 3] == 0).all() and (cal[:, :, :, 3] == 0).all()
    I = image(cal, freq, tau_pix, w, False, 1)
    assert np.abs(raw[:, :2, x0] - 1).min() > 0.05
    assert np.abs(I[:, :2, x0] - 1).max() < 1e-5 and (np.argmax(I[:, 0], axis=1) == x0).all() and (np.argmax(I[:, 1], axis=1) == x0).all()


def test_inverse_gains_reference_phase_and_apply_gains_identities():
    rng = np.random.default_rng(9)
    nfine, nstand = 3, 7
    g = rng.uniform(0.5, 2.0, (nfine, 2, nstand)) * np.exp(2j * np.pi * rng.uniform(size=(nfine, 2, nstand)))
    g[:, :, 4] = 0
    inv = inverse_gains(g)
    assert inv.shape == (nfine, 2 * nstand) and inv.flags['C_CONTIGUOUS'] and (inv[:, 8:10] == 0).all()
    gi = g.transpose(0, 2, 1).reshape(nfine, -1)                # per input 2 s + p
    assert np.allclose((inv * gi)[:, gi[0] != 0], 1.0, rtol=0, atol=1e-15)
    r = reference_phase(g, 2)
    assert np.abs(r[:, :, 2].imag).max() < 1e-15 and (r[:, :, 2].real > 0).all() and np.allclose(np.abs(r), np.abs(g))
    assert np.allclose(r[:, :, :, None] * np.conj(r[:, :, None, :]), g[:, :, :, None] * np.conj(g[:, :, None, :]))    # g g^H keeps its value
    assert np.array_equal(reference_phase(g, 4), g)            # (a reference of gain 0 leaves them alone)
    assert np.allclose(reference_phase(r, 2), r)
    M = rng.standard_normal((nfine, nstand, 2, nstand, 2)) + 1j * rng.standard_normal((nfine, nstand, 2, nstand, 2))
    V = gi.reshape(nfine, nstand, 2)[:, :, :, None, None] * np.conj(gi.reshape(nfine, nstand, 2))[:, None, None, :, :] * M
    back = apply_gains(V, g)
    live = np.arange(nstand) != 4
    assert np.allclose(back[:, live][:, :, :, live], M[:, live][:, :, :, live]) and (back[:, 4] == 0).all() and (back[:, :, :, 4] == 0).all()
    again = apply_gains(V, r)                                   # a phase per (channel, pol) cancels in the parallel hands ...
    assert all(np.allclose(again[:, :, p, :, p], back[:, :, p, :, p]) for p in (0, 1))
    assert not np.allclose(again[:, :, 0, :, 1], back[:, :, 0, :, 1])      # ... and not in the cross hands: the X-Y phase is undetermined
    for bad in (g[0], g[:, :1]):
        with pytest.raises(ValueError):
            inverse_gains(bad)
    with pytest.raises(ValueError):
        apply_gains(V[:, :3], g)
    with pytest.raises(ValueError, match="reference_phase"):
        reference_phase(g, nstand)


# ---------------------------------------------------------------- the block on CPU rings
NSTAND, NFINE, NSRC, ACC_LEN, NITER, TOL = 6, 2, 2, 96, 30, 1e-5


class GaincalBackend(OracleBackend):
    """The oracle backend plus xengGaincal* served by the complex64 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.gc, self.calls, self.keep = None, [], None
        self.tau = self.freq = self.flux = self.w = None
        self.niter, self.tol = 60, 1e-5

    def gaincal_initialize(self, gpu, nstand, nfine, nsrc):
        if nsrc > 32 or nstand > 512:
            return 1
        self.gc = dict(nstand=nstand, nfine=nfine, nsrc=nsrc)
        self.tau = self.w = self.keep = None
        self.calls.append('init')
        return 0

    def gaincal_set_model(self, tau, freq, flux):
        u = self.gc
        self.tau = np.array(tau, np.float64).reshape(u['nsrc'], u['nstand'])
        self.freq = np.array(freq, np.float64).reshape(u['nfine'])
        assert flux.dtype == np.float32
        self.flux = np.array(flux).reshape(u['nfine'], u['nsrc'])
        self.keep = None
        self.calls.append('model')
        return 0

    def gaincal_set_weights(self, weights, refant):
        if not weights[refant] > 0:
            return 1
        self.w, self.refant, self.keep = np.array(weights, np.float32).reshape(self.gc['nstand']), refant, None
        self.calls.append('weights')
        return 0

    def gaincal_set_solver(self, niter, tol):
        self.niter, self.tol = niter, tol
        self.calls.append('solver')
        return 0

    def gaincal_run(self, vis_arr, out_arr, stats_offset, warm):
        u = self.gc
        if self.tau is None or self.w is None:
            return 2
        V = vis_arr.numpy().reshape(-1).view(np.uint8).view(np.complex64).reshape(u['nfine'], u['nstand'], 2, u['nstand'], 2)
        g, st, self.keep = solve(V, self.freq, self.tau, self.flux, self.w, self.refant, self.niter, self.tol, np.complex64, start=self.keep if warm else None)
        out = out_arr.numpy().reshape(-1).view(np.uint8)
        assert stats_offset == g.nbytes
        out[:g.nbytes] = np.ascontiguousarray(g).reshape(-1).view(np.uint8)
        out[g.nbytes:g.nbytes + st.size * 4] = st.astype(np.float32).reshape(-1).view(np.uint8)
        self.calls.append('run-warm' if warm else 'run')
        return 0

    def gaincal_mark(self):
        return self.beam_mark()

    def gaincal_wait(self, ticket):
        self.beam_wait(ticket)

    def gaincal_sync(self):
        pass


def vis_header(nstand=NSTAND, nfine=NFINE, seq0=0, fine_sfreq=50e6, **extra):
    """The sequence header UpchanCorr writes (upchan_corr_block.py output_header)."""
    hdr = source_header(nfine // 2, nstand, 2, seq0=seq0, sfreq=fine_sfreq + FINE_BW)
    hdr.update(nupchan=2, fine_lo=0, nfine=nfine, fine_bw_hz=FINE_BW, fine_sfreq=fine_sfreq, nframe_per_integration=ACC_LEN // 2, acc_len=ACC_LEN,
               complex=True, nbit=32)
    hdr.update(extra)
    return hdr


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


def _geometry(seed=11):
    rng = np.random.default_rng(seed)
    return random_array(rng, NSTAND, 300.0), sky(rng, NSRC)


FLUX = [3.0, 1.0]


def _block(iring, oring, be, **kw):
    pos, lmn = _geometry()
    args = dict(positions=pos, src_lmn=lmn, flux=FLUX, niter=NITER, tol=TOL)
    args.update(kw)
    return UpchanGainCal(LOG, iring, oring, backend=be, **args)


OSPAN = NFINE * 2 * NSTAND * 8 + NFINE * 2 * 4 * 4


def _split(span):
    raw = np.asarray(span).view(np.uint8).reshape(-1)
    ng = NFINE * 2 * NSTAND * 8
    return raw[:ng].view(np.complex64).reshape(NFINE, 2, NSTAND), raw[ng:].view(np.float32).reshape(NFINE, 2, 4)


def _integrations(rng, n, fine_sfreq):
    """n integrations of one sky through one set of gains, each with noise of its own: complex64 [n][NFINE][NSTAND][2][NSTAND][2]"""
    pos, lmn = _geometry()
    freq = fine_sfreq + FINE_BW * np.arange(NFINE)
    g = rng.uniform(0.5, 2.0, (NFINE, 2, NSTAND)) * np.exp(2j * np.pi * rng.uniform(size=(NFINE, 2, NSTAND)))
    V0 = corrupt(model_visibilities(freq, steering_delays(pos, lmn), FLUX), g)
    return np.array([noisy(rng, V0, 1e-4) for _ in range(n)]), freq


def _expected(chain, tau):
    """The restatement over a list of (V, freq, flux, w, refant, warm): what the block must have written, the keep carried along."""
    out, keep = [], None
    for V, freq, flux, w, refant, warm in chain:
        g, st, keep = solve(V, freq, tau, np.asarray(flux, np.float32), w, refant, NITER, TOL, np.complex64, start=keep if warm else None)
        out.append((g, st.astype(np.float32)))
    return out


def test_block_one_span_per_integration_header_and_warm_start(ring_impl):
    """Source -> UpchanGainCal -> Sink, two sequences of three integrations: every output span is the complex64 restatement of its
    input span with the sequence's own frequencies, the first of a sequence from a cold start and the others from the one before
    (which takes fewer iterations); the header is the input's plus nsrc, refant, niter, tol, stats_offset, nbit 32 and complex True;
    the model is set once per sequence."""
    rng = np.random.default_rng(13)
    pos, lmn = _geometry()
    tau = steering_delays(pos, lmn)
    hdrs = [vis_header(seq0=1000, fine_sfreq=50e6), vis_header(seq0=5000, fine_sfreq=62e6)]
    Vs, freqs = zip(*[_integrations(rng, 3, h['fine_sfreq']) for h in hdrs])
    span = NFINE * (2 * NSTAND) ** 2 * 8
    r0, r1 = Ring("uc-output"), Ring("gaincal-output")
    be = GaincalBackend()
    gc = _block(r0, r1, be, refant=1)
    sink = Sink(r1, OSPAN)
    run_blocks([gc], Source(r0, [(hdrs[s], Vs[s].reshape(-1).view(np.uint8), span) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    ones = np.ones(NSTAND, np.float32)
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        exp = _expected([(Vs[s][k], freqs[s], FLUX, ones, 1, k > 0) for k in range(3)], tau)
        assert len(spans) == 3
        for k in range(3):
            g, st = _split(spans[k])
            assert g.tobytes() == exp[k][0].tobytes() and st.tobytes() == exp[k][1].tobytes()
            assert (st[:, :, 3] == 1).all() and (st[:, :, 2] == NSTAND).all()
        assert (_split(spans[1])[1][:, :, 0] < _split(spans[0])[1][:, :, 0]).all()
        assert tag == hd['seq0'] == hdrs[s]['seq0']
        assert (hd['nsrc'], hd['refant'], hd['niter'], hd['tol'], hd['stats_offset'], hd['nbit'], hd['complex']) == (NSRC, 1, NITER, TOL, NFINE * 2 * NSTAND * 8, 32, True)
        assert all(hd[k] == hdrs[s][k] for k in ('nfine', 'fine_sfreq', 'fine_bw_hz', 'nstand', 'npol', 'acc_len', 'nupchan'))
    assert be.calls == ['init', 'solver', 'weights', 'model', 'run', 'run-warm', 'run-warm', 'model', 'run', 'run-warm', 'run-warm']
    assert gc.stats['nsolve'] == 6 and gc.stats['ngap'] == 0


def test_block_commands_at_the_next_integration_and_a_gap_forces_a_cold_start(ring_impl):
    """Integrations 0..7 of a sequence, 3 never read.  set_weights before 1 (flagging stand 2, whose visibilities are NaN from then
    on): 0 carries the constructor's weights, 1 starts cold with the new ones, 2 warm.  The gap ends the output sequence and 4 starts
    cold.  A `flux` command before 5 (a cold start, the same sequence); a `refant` command before 6 starts a sequence of its own
    whose header names the new stand; a refant of weight 0 before 7 is refused at the integration and changes nothing.  What is not
    a list of nstand finite numbers >= 0, a stand in range or fluxes >= 0 is refused as a command and changes nothing."""
    rng = np.random.default_rng(17)
    pos, lmn = _geometry()
    tau = steering_delays(pos, lmn)
    hdr = vis_header(seq0=960)
    V, freq = _integrations(rng, 8, hdr['fine_sfreq'])
    V[1:, :, 2] = np.nan
    V[1:, :, :, :, 2] = np.nan
    w0 = np.array([1, 2, 1, 0.5, 1, 1], np.float32)
    w1 = np.array([2, 1, 0, 1, 3, 1], np.float32)
    f1 = [[2.0, 1.5], [2.5, 0.5]]
    box = {}

    def spans():
        for k in (0, 1, 2, 4, 5, 6, 7):
            im = box['gc']
            if k == 1:
                im.set_weights(w1)
                for bad in ([1.0] * 5, [1, 1, 1, 1, 1, -1], [1, 1, 1, 1, 1, np.nan]):
                    with pytest.raises(ValueError, match="UPCHAN_GAINCAL"):
                        im.set_weights(bad)
                for bad in (-1, NSTAND, 1.5, True):
                    with pytest.raises(ValueError, match="UPCHAN_GAINCAL"):
                        im.set_refant(bad)
                for bad in ([1.0], [1.0, -1.0], [[1.0, 1.0]] * 3, "none"):
                    with pytest.raises(ValueError, match="UPCHAN_GAINCAL"):
                        im.set_flux(bad)
            if k == 5:
                im.process_command_strings(_cmd(flux=f1))
                assert im.last_response['val']['status'] == 'normal'
                for n, bad in enumerate(({'weights': [1.0]}, {'weights': "none"}, {'weights': [1, 1, 1, 1, 1, -2.0]}, {'refant': NSTAND}, {'refant': -1},
                                         {'refant': 1.5}, {'flux': [1.0]}, {'flux': [1.0, -1.0]}, {'flux': [[1.0, 1.0]] * 3})):
                    im.process_command_strings(_cmd(str(2 + n), **bad))
                    assert im.last_response['val']['status'] == 'error', bad
            if k == 6:
                im.process_command_strings(_cmd("20", refant=4))
                assert im.last_response['val']['status'] == 'normal'
            if k == 7:
                im.set_refant(2)                    # (weight 0 since integration 1)
            yield k, V[k]

    be = GaincalBackend()
    r1 = Ring("gaincal-output")
    gc = box['gc'] = _block(_FakeRing([_FakeSeq(hdr, spans(), NFINE * (2 * NSTAND) ** 2 * 8)]), r1, be, weights=w0)
    sink = Sink(r1, OSPAN)
    sink.start()
    gc.main()
    sink.join(20)
    (h0, t0, a), (h1, t1, b), (h2, t2, c) = sink.sequences
    assert (h0['seq0'], t0, h1['seq0'], t1, h2['seq0'], t2) == (960, 960, 960 + 4 * ACC_LEN, 960 + 4 * ACC_LEN, 960 + 6 * ACC_LEN, 960 + 6 * ACC_LEN)
    assert (h0['refant'], h1['refant'], h2['refant']) == (0, 0, 4)
    exp = _expected([(V[0], freq, FLUX, w0, 0, False), (V[1], freq, FLUX, w1, 0, False), (V[2], freq, FLUX, w1, 0, True), (V[4], freq, FLUX, w1, 0, False),
                     (V[5], freq, f1, w1, 0, False), (V[6], freq, f1, w1, 4, False), (V[7], freq, f1, w1, 4, True)], tau)
    assert (len(a), len(b), len(c)) == (3, 2, 2)
    for k, sp in enumerate(list(a) + list(b) + list(c)):
        g, st = _split(sp)
        assert g.tobytes() == exp[k][0].tobytes() and st.tobytes() == exp[k][1].tobytes(), k
        assert np.isfinite(g.view(np.float32)).all() and (k == 0 or ((g[:, :, 2] == 0).all() and (st[:, :, 2] == NSTAND - 1).all()))
    assert be.calls == ['init', 'solver', 'weights', 'model', 'run', 'weights', 'run', 'run-warm', 'run', 'model', 'run', 'weights', 'run', 'run-warm']
    assert gc.stats['ngap'] == 1 and gc.stats['nsolve'] == 7


def test_block_without_warm_start_starts_every_integration_cold():
    rng = np.random.default_rng(19)
    hdr = vis_header(seq0=0)
    V, freq = _integrations(rng, 3, hdr['fine_sfreq'])
    be = GaincalBackend()
    r1 = Ring("gaincal-output")
    gc = _block(_FakeRing([_FakeSeq(hdr, [(k, V[k]) for k in range(3)], NFINE * (2 * NSTAND) ** 2 * 8)]), r1, be, warm_start=False)
    sink = Sink(r1, OSPAN)
    sink.start()
    gc.main()
    sink.join(20)
    assert be.calls == ['init', 'solver', 'weights', 'model', 'run', 'run', 'run']


@pytest.mark.parametrize("kw", [dict(niter=-1), dict(niter=1025), dict(niter=1.5), dict(tol=-1e-3), dict(tol=np.nan), dict(weights=[1.0] * 5),
                                dict(weights=[1, 1, 1, 1, 1, -1.0]), dict(weights=[0, 1, 1, 1, 1, 1.0]), dict(refant=6), dict(refant=-1), dict(refant=1.0),
                                dict(flux=[1.0]), dict(flux=[1.0, -2.0]), dict(flux=[1.0, np.inf]), dict(src_lmn=[[0, 0]]), dict(positions=np.zeros((6, 2))),
                                dict(src_lmn=np.tile([0.0, 0.0, 1.0], (33, 1)))])
def test_constructor_refuses_bad_arguments(kw):
    be = GaincalBackend()
    with pytest.raises(ValueError, match="UPCHAN_GAINCAL"):
        _block(Ring("a"), Ring("b"), be, **kw)
    assert be.gc is None
    _block(Ring("a"), Ring("b"), be, weights=[0, 1, 1, 1, 1, 1.0], refant=1, niter=0, tol=0)


@pytest.mark.parametrize("bad", [dict(npol=1), dict(nstand=7), dict(nfine=None), dict(nfine=0), dict(nbit=8), dict(complex=False), dict(fine_sfreq=None),
                                 dict(fine_bw_hz=0.0), dict(npix=7), dict(nsrc=2), dict(acc_len=0), dict(flux=[[1.0, 1.0]] * 3)])
def test_block_refuses_what_is_not_its_visibilities(bad):
    """npol != 2, a stand count that differs from the positions', fluxes per channel for another channel count, and headers that
    are not UpchanCorr's: refused at the sequence, before anything is run."""
    be = GaincalBackend()
    hdr = vis_header()
    kw = {}
    for k, v in bad.items():
        if k == 'flux':
            kw['flux'] = v
        elif v is None:
            del hdr[k]
        else:
            hdr[k] = v
    x = np.zeros((NFINE, NSTAND, 2, NSTAND, 2), np.complex64)
    gc = _block(_FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), be, **kw)
    with pytest.raises(ValueError, match="UPCHAN_GAINCAL"):
        gc.main()
    assert 'run' not in be.calls


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengGaincalInitialize", "xengGaincalGetInfo", "xengGaincalSetModel", "xengGaincalSetWeights", "xengGaincalSetSolver", "xengGaincalRun",
         "xengGaincalCheckGuards", "xengGaincalMark", "xengGaincalWait", "xengGaincalTicketDone", "xengGaincalSync", "xengGaincalDestroy")


def test_backend_forwards_every_call_the_block_makes():
    """Every gaincal_* method of the real backend exists, and reaches the C entry point of its name with the arguments in order
    (a recording library in the place of libxeng.so)."""
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("gaincal_initialize", "gaincal_set_model", "gaincal_set_weights", "gaincal_set_solver", "gaincal_run", "gaincal_info", "gaincal_guards_intact",
              "gaincal_mark", "gaincal_wait", "gaincal_sync"):
        assert callable(getattr(HipBackend, m)), m
    for m in ("gaincal_initialize", "gaincal_set_model", "gaincal_set_weights", "gaincal_set_solver", "gaincal_run", "gaincal_mark", "gaincal_wait", "gaincal_sync"):
        assert callable(getattr(GaincalBackend, m)), m

    class Recorder:
        def __init__(self):
            self.seen = []

        def __getattr__(self, name):
            def f(*args):
                self.seen.append((name, args))
                return 0
            return f

    class Arr:
        ptr = 4096

    be = HipBackend.__new__(HipBackend)
    be._lib = be._enq = rec = Recorder()
    tau, freq, flux, w = np.zeros((2, 6)), np.zeros(3), np.ones((3, 2), np.float32), np.ones(6, np.float32)
    assert be.gaincal_initialize(0, 6, 3, 2) == 0 and be.gaincal_set_model(tau, freq, flux) == 0 and be.gaincal_set_weights(w, 4) == 0
    assert be.gaincal_set_solver(30, 1e-5) == 0 and be.gaincal_run(Arr, Arr, 288, True) == 0
    names = [n for n, _ in rec.seen]
    assert names == ["xengGaincalInitialize", "xengGaincalSetModel", "xengGaincalSetWeights", "xengGaincalSetSolver", "xengGaincalRun"]
    assert rec.seen[0][1] == (0, 6, 3, 2) and rec.seen[2][1][1] == 4 and rec.seen[3][1] == (30, 1e-5) and rec.seen[4][1] == (4096, 4096, 4096 + 288, 1)
    for bad in ((tau.astype(np.float32), freq, flux), (tau, freq, flux.astype(np.float64)), (tau[:, ::2], freq, flux)):
        with pytest.raises(TypeError, match="gaincal_set_model"):
            be.gaincal_set_model(*bad)
    with pytest.raises(TypeError, match="gaincal_set_weights"):
        be.gaincal_set_weights(w.astype(np.float64), 0)


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Mark and TicketDone are enqueue-only, the calls that wait are not.  Initialize
    refuses every size outside the contract before it touches a device; Run refuses null and misaligned pointers, the getters null
    results, SetModel and SetWeights null tables, SetSolver what is outside its limits, before looking for a context; without one,
    INVALID_STATE."""
    lib = ffi.lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in ffi.SYMBOLS, name
    for name in ("xengGaincalRun", "xengGaincalMark", "xengGaincalTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengGaincalInitialize", "xengGaincalSetModel", "xengGaincalSetWeights", "xengGaincalSetSolver", "xengGaincalWait", "xengGaincalSync",
                 "xengGaincalCheckGuards", "xengGaincalGetInfo"):
        assert name not in ffi.ENQUEUE_ONLY, name
    good = (0, 352, 96, 8)                      # (gpu, nstand, nfine, nsrc)
    for i, v in ((1, 0), (1, -3), (1, 513), (2, 0), (2, 65536), (3, 0), (3, 33)):
        args = list(good)
        args[i] = v
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengGaincalInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    s, d = ctypes.c_int(), ctypes.c_double()
    f64 = np.zeros(4, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    f32 = np.ones(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for name, args in (("xengGaincalRun", (None, 4096, 4096, 0)), ("xengGaincalRun", (4096, None, 4096, 0)), ("xengGaincalRun", (4096, 4096, None, 0)),
                       ("xengGaincalRun", (4104, 4096, 4096, 0)), ("xengGaincalRun", (4096, 4100, 4096, 0)), ("xengGaincalRun", (4096, 4096, 4098, 0)),
                       ("xengGaincalGetInfo", (None, ctypes.byref(s), ctypes.byref(d), ctypes.byref(s))),
                       ("xengGaincalGetInfo", (ctypes.byref(s), None, ctypes.byref(d), ctypes.byref(s))),
                       ("xengGaincalGetInfo", (ctypes.byref(s), ctypes.byref(s), None, ctypes.byref(s))),
                       ("xengGaincalGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(d), None)),
                       ("xengGaincalSetModel", (None, f64, f32)), ("xengGaincalSetModel", (f64, None, f32)), ("xengGaincalSetModel", (f64, f64, None)),
                       ("xengGaincalSetWeights", (None, 0)), ("xengGaincalSetSolver", (-1, 1e-5)), ("xengGaincalSetSolver", (1025, 1e-5)),
                       ("xengGaincalSetSolver", (10, -1e-5)), ("xengGaincalSetSolver", (10, float('nan'))),
                       ("xengGaincalMark", (None,)), ("xengGaincalTicketDone", (1, None)), ("xengGaincalCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_gaincal_gpu.py covers the rest)
    t = ctypes.c_ulonglong()
    for name, args in (("xengGaincalRun", (4096, 4096, 4096, 0)), ("xengGaincalSetModel", (f64, f64, f32)), ("xengGaincalSetWeights", (f32, 1)),
                       ("xengGaincalSetSolver", (10, 1e-5)), ("xengGaincalGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(d), ctypes.byref(s))),
                       ("xengGaincalMark", (ctypes.byref(t),)), ("xengGaincalWait", (1,)), ("xengGaincalTicketDone", (1, ctypes.byref(s))),
                       ("xengGaincalSync", ()), ("xengGaincalCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengGaincalDestroy")      # (nothing to destroy: success)
