"""UpchanCalApply without a GPU: the restatement (tests/calapply_ref.py) against apply_gains and model_visibilities of
blocks/calibration.py; the block on CPU rings (both implementations) with a backend, defined here, that serves calapply_* from the
complex64 restatement -- one span per span, the header keys and who accepts them, set_gains / set_flux / the flux command at the
next integration, a gap, the refusals -- and the C entry points' argument checks."""
import ctypes
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import UpchanCalApply, UpchanGainCal, UpchanImage, apply_gains, model_visibilities, steering_delays
from caltech_bifrost_dsp_amd.ring import Ring
from tests.calapply_ref import apply, case, factors, hermitian_bits
from tests.fake_backend import OracleBackend
from tests.gaincal_ref import sky
from tests.image_ref import hermitian_uneven, random_array
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
FINE_BW = 23925.78125 / 2


@pytest.fixture(params=["native", "python"])
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape", [(22, 1, 3), (35, 3, 2), (35, 0, 2)])
def test_restatement_is_apply_gains_minus_the_model_in_float64(shape):
    """With h = inverse_gains(g) unrounded, the restatement's lower triangle and diagonal are apply_gains(V, g) minus
    model_visibilities on the pp blocks, to rounding (measured 4e-16 of the word's scale; asserted at 1e-13); its upper triangle is
    the conjugate of its lower and its diagonal is real; rows and columns without a gain are zeros whatever they held."""
    nstand, nsrc, nfine = shape
    tau, freq, flux, h, V = case(*shape)
    rng = np.random.default_rng(3)
    g = rng.uniform(0.5, 2.0, (nfine, 2, nstand)) * np.exp(2j * np.pi * rng.uniform(size=(nfine, 2, nstand)))
    g[:, :, 3] = 0
    g[:, 1, 5] = 0
    V = V.copy()
    V[:, 3] = np.nan
    V[:, :, :, 3] = np.inf
    h64 = np.where(g != 0, 1.0 / np.where(g != 0, g, 1), 0)
    got = apply(V, h64, freq, tau, flux)
    exp = apply_gains(V, g)
    if nsrc:
        M = model_visibilities(freq, tau, flux)
        live = g != 0
        for p in range(2):
            exp[:, :, p, :, p] -= np.where(live[:, p, :, None] & live[:, p, None, :], M, 0)
    n = 2 * nstand
    low = np.tril(np.ones((n, n), bool), -1)
    G, E = got.reshape(nfine, n, n), exp.reshape(nfine, n, n)
    assert np.isfinite(G).all()
    assert np.abs(G[:, low] - E[:, low]).max() <= 1e-13 * np.abs(E).max()
    assert np.abs(np.einsum('cii->ci', G) - np.einsum('cii->ci', E).real).max() <= 1e-13 * np.abs(E).max()
    assert np.array_equal(G, np.conj(G.transpose(0, 2, 1))) and (got[:, 3] == 0).all() and (got[:, :, :, 5, 1] == 0).all()
    assert hermitian_bits(apply(V, factors(g), freq, tau, flux, np.complex64))
    assert factors(g).dtype == np.complex64 and factors(g).shape == (nfine, 2, nstand) and (factors(g)[:, 1, 5] == 0).all()


# ---------------------------------------------------------------- the block on CPU rings
NSTAND, NFINE, NSRC, ACC_LEN = 6, 2, 2, 96
SPAN = NFINE * (2 * NSTAND) ** 2 * 8
FLUX = [3.0, 1.0]


class CalapplyBackend(OracleBackend):
    """The oracle backend plus xengCalapply* served by the complex64 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.ca, self.calls = None, []
        self.tau = self.freq = self.flux = self.h = None

    def calapply_initialize(self, gpu, nstand, nfine, nsrc):
        if nsrc > 32 or nstand > 512:
            return 1
        self.ca = dict(nstand=nstand, nfine=nfine, nsrc=nsrc)
        self.tau = self.freq = None
        self.h = np.ones((nfine, 2, nstand), np.complex64)
        self.calls.append('init')
        return 0

    def calapply_set_model(self, tau, freq, flux):
        u = self.ca
        assert (tau is None) == (u['nsrc'] == 0) == (flux is None)
        self.freq = np.array(freq, np.float64).reshape(u['nfine'])
        if u['nsrc']:
            assert flux.dtype == np.float32
            self.tau = np.array(tau, np.float64).reshape(u['nsrc'], u['nstand'])
            self.flux = np.array(flux).reshape(u['nfine'], u['nsrc'])
        self.calls.append('model')
        return 0

    def calapply_set_factors(self, h):
        assert h.dtype == np.complex64 and h.shape == (self.ca['nfine'], 2, self.ca['nstand'])
        self.h = np.array(h)
        self.calls.append('factors')
        return 0

    def calapply_run(self, vis_arr, out_arr):
        u = self.ca
        if u['nsrc'] and self.tau is None:
            return 2
        V = vis_arr.numpy().reshape(-1).view(np.uint8).view(np.complex64).reshape(u['nfine'], u['nstand'], 2, u['nstand'], 2)
        y = np.ascontiguousarray(apply(V, self.h, self.freq, self.tau, self.flux, np.complex64))
        out_arr.numpy().reshape(-1).view(np.uint8)[:y.nbytes] = y.reshape(-1).view(np.uint8)
        self.calls.append('run')
        return 0

    def calapply_mark(self):
        return self.beam_mark()

    def calapply_wait(self, ticket):
        self.beam_wait(ticket)

    def calapply_sync(self):
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


def _gains(rng):
    g = rng.uniform(0.5, 2.0, (NFINE, 2, NSTAND)) * np.exp(2j * np.pi * rng.uniform(size=(NFINE, 2, NSTAND)))
    g[:, :, 4] = 0
    return g


def _block(iring, oring, be, **kw):
    pos, lmn = _geometry()
    args = dict(positions=pos, src_lmn=lmn, flux=FLUX)
    args.update(kw)
    return UpchanCalApply(LOG, iring, oring, backend=be, **args)


def _words(span):
    return np.asarray(span).view(np.uint8).reshape(-1).view(np.complex64).reshape(NFINE, NSTAND, 2, NSTAND, 2)


def _expect(V, h, freq, flux, tau):
    F = None if tau is None else np.ascontiguousarray(np.broadcast_to(np.asarray(flux, np.float32), (NFINE, NSRC)))
    return apply(V, np.ones((NFINE, 2, NSTAND), np.complex64) if h is None else h, freq, tau, F, np.complex64)


def test_block_one_span_per_span_and_header(ring_impl):
    """Source -> UpchanCalApply -> Sink, two sequences of three integrations, the second already calibrated with two sources
    subtracted: every output span is the complex64 restatement of its input span with the sequence's own frequencies and the
    constructor's gains; the header is the input's plus calibrated and nsubtracted (the input's count plus nsrc), without nsrc or
    npix, and UpchanImage and UpchanGainCal accept it; the model is set once per sequence, the factors once."""
    rng = np.random.default_rng(13)
    pos, lmn = _geometry()
    tau = steering_delays(pos, lmn)
    g = _gains(rng)
    hdrs = [vis_header(seq0=1000, fine_sfreq=50e6), vis_header(seq0=5000, fine_sfreq=62e6, calibrated=True, nsubtracted=2)]
    Vs = [hermitian_uneven(rng, 3 * NFINE, NSTAND).reshape(3, NFINE, NSTAND, 2, NSTAND, 2) for _ in hdrs]
    r0, r1 = Ring("uc-output"), Ring("calapply-output")
    be = CalapplyBackend()
    ca = _block(r0, r1, be, gains=g)
    sink = Sink(r1, SPAN)
    run_blocks([ca], Source(r0, [(hdrs[s], Vs[s].reshape(-1).view(np.uint8), SPAN) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        freq = hdrs[s]['fine_sfreq'] + FINE_BW * np.arange(NFINE)
        assert len(spans) == 3
        for k in range(3):
            got = _words(spans[k])
            assert got.tobytes() == _expect(Vs[s][k], factors(g), freq, FLUX, tau).astype(np.complex64).tobytes()
            assert (got[:, 4] == 0).all() and (got[:, :, :, 4] == 0).all()
        assert tag == hd['seq0'] == hdrs[s]['seq0']
        assert hd['calibrated'] is True and hd['nsubtracted'] == (NSRC, NSRC + 2)[s] and 'nsrc' not in hd and 'npix' not in hd
        assert all(hd[k] == hdrs[s][k] for k in ('nfine', 'fine_sfreq', 'fine_bw_hz', 'nstand', 'npol', 'acc_len', 'nupchan', 'nbit', 'complex'))
        # the consumers of UpchanCorr's ring take it unchanged
        im = UpchanImage(LOG, Ring("a"), Ring("b"), pos, lmn, backend=be)
        gc = UpchanGainCal(LOG, Ring("a"), Ring("b"), pos, lmn, FLUX, backend=be)
        assert im._check_header(hd) is not None and gc._check_header(hd) == (NFINE, ACC_LEN)
        assert _block(Ring("a"), Ring("b"), be)._check_header(hd) == (NFINE, ACC_LEN)
    assert be.calls == ['init', 'factors', 'model', 'run', 'run', 'run', 'model', 'run', 'run', 'run']
    assert ca.stats['napply'] == 6 and ca.stats['ngap'] == 0


def test_block_controls_at_the_next_integration_and_a_gap_opens_a_new_sequence(ring_impl):
    """Integrations 0..6 of a sequence, 3 never read, from a block without gains.  set_gains before 1: 0 carries unit factors, 1
    the new ones.  set_flux before 2.  The gap ends the output sequence; 4 opens one whose header starts there.  A `flux` command
    before 5; set_factors before 6.  What is not [nfine][2][nstand] finite gains or factors, or fluxes >= 0, is refused where it
    is given and changes nothing."""
    rng = np.random.default_rng(17)
    pos, lmn = _geometry()
    tau = steering_delays(pos, lmn)
    hdr = vis_header(seq0=960)
    freq = hdr['fine_sfreq'] + FINE_BW * np.arange(NFINE)
    V = hermitian_uneven(rng, 7 * NFINE, NSTAND).reshape(7, NFINE, NSTAND, 2, NSTAND, 2)
    g = _gains(rng)
    f1, f2 = [[2.0, 1.5], [2.5, 0.5]], [0.5, 4.0]
    h2 = (rng.standard_normal((NFINE, 2, NSTAND)) + 1j * rng.standard_normal((NFINE, 2, NSTAND))).astype(np.complex64)
    box = {}

    def spans():
        for k in (0, 1, 2, 4, 5, 6):
            ca = box['ca']
            if k == 1:
                ca.set_gains(g)
                for bad in (g[0], g[:, :, :5], g[:1], np.where(np.arange(NSTAND) == 2, np.nan, g), "none"):
                    with pytest.raises(ValueError, match="UPCHAN_CALAPPLY"):
                        ca.set_gains(bad)
                for bad in (h2[0], h2[:, :1], np.where(np.arange(NSTAND) == 2, np.inf, h2)):
                    with pytest.raises(ValueError, match="UPCHAN_CALAPPLY"):
                        ca.set_factors(bad)
                for bad in ([1.0], [1.0, -1.0], [[1.0, 1.0]] * 3, "none"):
                    with pytest.raises(ValueError, match="UPCHAN_CALAPPLY"):
                        ca.set_flux(bad)
            if k == 2:
                ca.set_flux(f1)
            if k == 5:
                ca.process_command_strings(_cmd(flux=f2))
                assert ca.last_response['val']['status'] == 'normal'
                for n, bad in enumerate(({'flux': [1.0]}, {'flux': [1.0, -1.0]}, {'flux': [[1.0, 1.0]] * 3})):
                    ca.process_command_strings(_cmd(str(2 + n), **bad))
                    assert ca.last_response['val']['status'] == 'error', bad
            if k == 6:
                ca.set_factors(h2)
            yield k, V[k]

    be = CalapplyBackend()
    r1 = Ring("calapply-output")
    ca = box['ca'] = _block(_FakeRing([_FakeSeq(hdr, spans(), SPAN)]), r1, be)
    sink = Sink(r1, SPAN)
    sink.start()
    ca.main()
    sink.join(20)
    (h0, t0, a), (h1, t1, b) = sink.sequences
    assert (h0['seq0'], t0, h1['seq0'], t1) == (960, 960, 960 + 4 * ACC_LEN, 960 + 4 * ACC_LEN)
    assert (len(a), len(b)) == (3, 3) and h1['nsubtracted'] == NSRC and h1['calibrated'] is True
    hg = factors(g)
    chain = [(V[0], None, FLUX), (V[1], hg, FLUX), (V[2], hg, f1), (V[4], hg, f1), (V[5], hg, f2), (V[6], h2, f2)]
    for k, sp in enumerate(list(a) + list(b)):
        assert _words(sp).tobytes() == _expect(chain[k][0], chain[k][1], freq, chain[k][2], tau).astype(np.complex64).tobytes(), k
    assert be.calls == ['init', 'factors', 'model', 'run', 'factors', 'run', 'model', 'run', 'run', 'model', 'run', 'factors', 'run']
    assert ca.stats['ngap'] == 1 and ca.stats['napply'] == 6


def test_block_without_sources_only_calibrates():
    rng = np.random.default_rng(19)
    pos, _ = _geometry()
    hdr = vis_header(seq0=0, nsubtracted=1, calibrated=True)
    freq = hdr['fine_sfreq'] + FINE_BW * np.arange(NFINE)
    V = hermitian_uneven(rng, 2 * NFINE, NSTAND).reshape(2, NFINE, NSTAND, 2, NSTAND, 2)
    g = _gains(rng)
    be = CalapplyBackend()
    r1 = Ring("calapply-output")
    ca = UpchanCalApply(LOG, _FakeRing([_FakeSeq(hdr, [(k, V[k]) for k in range(2)], SPAN)]), r1, pos, gains=g, backend=be)
    sink = Sink(r1, SPAN)
    sink.start()
    ca.main()
    sink.join(20)
    (hd, _, spans), = sink.sequences
    assert hd['nsubtracted'] == 1 and be.ca['nsrc'] == 0 and be.calls == ['init', 'factors', 'model', 'run', 'run']
    for k in range(2):
        assert _words(spans[k]).tobytes() == _expect(V[k], factors(g), freq, None, None).astype(np.complex64).tobytes()
    with pytest.raises(ValueError, match="UPCHAN_CALAPPLY"):
        ca.set_flux([1.0])


@pytest.mark.parametrize("kw", [dict(flux=[1.0]), dict(flux=[1.0, -2.0]), dict(flux=[1.0, np.inf]), dict(flux=None), dict(src_lmn=[[0, 0]]),
                                dict(positions=np.zeros((6, 2))), dict(src_lmn=np.tile([0.0, 0.0, 1.0], (33, 1)), flux=[1.0] * 33),
                                dict(src_lmn=None), dict(gains=np.ones((2, 6))), dict(gains=np.ones((2, 2, 5))), dict(gains=np.full((2, 2, 6), np.inf)),
                                dict(gains="none")])
def test_constructor_refuses_bad_arguments(kw):
    """(src_lmn = None with fluxes left in place: fluxes without directions)"""
    be = CalapplyBackend()
    with pytest.raises(ValueError, match="UPCHAN_CALAPPLY"):
        _block(Ring("a"), Ring("b"), be, **kw)
    assert be.ca is None
    _block(Ring("a"), Ring("b"), be, src_lmn=None, flux=None, gains=np.ones((NFINE, 2, NSTAND)))


@pytest.mark.parametrize("bad", [dict(npol=1), dict(nstand=7), dict(nfine=None), dict(nfine=0), dict(nbit=8), dict(complex=False), dict(fine_sfreq=None),
                                 dict(fine_bw_hz=0.0), dict(npix=7), dict(nsrc=2), dict(acc_len=0), dict(nsubtracted=-1), dict(flux=[[1.0, 1.0]] * 3),
                                 dict(gains=np.ones((3, 2, 6)))])
def test_block_refuses_what_is_not_its_visibilities(bad):
    """npol != 2, a stand count that differs from the positions', fluxes or gains per channel for another channel count, and headers
    that are not UpchanCorr's or this block's: refused at the sequence, before anything is run."""
    be = CalapplyBackend()
    hdr = vis_header()
    kw = {}
    for k, v in bad.items():
        if k in ('flux', 'gains'):
            kw[k] = v
        elif v is None:
            del hdr[k]
        else:
            hdr[k] = v
    x = np.zeros((NFINE, NSTAND, 2, NSTAND, 2), np.complex64)
    ca = _block(_FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), be, **kw)
    with pytest.raises(ValueError, match="UPCHAN_CALAPPLY"):
        ca.main()
    assert 'run' not in be.calls


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengCalapplyInitialize", "xengCalapplyGetInfo", "xengCalapplySetModel", "xengCalapplySetFactors", "xengCalapplyRun", "xengCalapplyCheckGuards",
         "xengCalapplyMark", "xengCalapplyWait", "xengCalapplyTicketDone", "xengCalapplySync", "xengCalapplyDestroy")


def test_backend_forwards_every_call_the_block_makes():
    """Every calapply_* method of the real backend exists, and reaches the C entry point of its name with the arguments in order
    (a recording library in the place of libxeng.so)."""
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("calapply_initialize", "calapply_set_model", "calapply_set_factors", "calapply_run", "calapply_info", "calapply_guards_intact", "calapply_mark",
              "calapply_wait", "calapply_sync"):
        assert callable(getattr(HipBackend, m)), m
    for m in ("calapply_initialize", "calapply_set_model", "calapply_set_factors", "calapply_run", "calapply_mark", "calapply_wait", "calapply_sync"):
        assert callable(getattr(CalapplyBackend, m)), m

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
    tau, freq, flux, h = np.zeros((2, 6)), np.zeros(3), np.ones((3, 2), np.float32), np.ones((3, 2, 6), np.complex64)
    assert be.calapply_initialize(0, 6, 3, 2) == 0 and be.calapply_set_model(tau, freq, flux) == 0 and be.calapply_set_factors(h) == 0
    assert be.calapply_set_model(None, freq, None) == 0 and be.calapply_run(Arr, Arr) == 0
    names = [n for n, _ in rec.seen]
    assert names == ["xengCalapplyInitialize", "xengCalapplySetModel", "xengCalapplySetFactors", "xengCalapplySetModel", "xengCalapplyRun"]
    assert rec.seen[0][1] == (0, 6, 3, 2) and rec.seen[4][1] == (4096, 4096)
    assert rec.seen[1][1][0] is not None and rec.seen[1][1][2] is not None and rec.seen[3][1][0] is None and rec.seen[3][1][2] is None
    assert rec.seen[2][1][0].value == h.ctypes.data
    for bad in ((tau.astype(np.float32), freq, flux), (tau, freq, flux.astype(np.float64)), (tau[:, ::2], freq, flux), (tau, None, flux)):
        with pytest.raises(TypeError, match="calapply_set_model"):
            be.calapply_set_model(*bad)
    for bad in (h.astype(np.complex128), h[:, :, ::2], h.view(np.float32)):
        with pytest.raises(TypeError, match="calapply_set_factors"):
            be.calapply_set_factors(bad)


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Mark and TicketDone are enqueue-only, the calls that wait are not.  Initialize
    refuses every size outside the contract before it touches a device; Run refuses null and misaligned pointers, the getters null
    results, SetModel null frequencies and SetFactors null factors, before looking for a context; without one, INVALID_STATE."""
    lib = ffi.lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in ffi.SYMBOLS, name
    for name in ("xengCalapplyRun", "xengCalapplyMark", "xengCalapplyTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengCalapplyInitialize", "xengCalapplySetModel", "xengCalapplySetFactors", "xengCalapplyWait", "xengCalapplySync", "xengCalapplyCheckGuards",
                 "xengCalapplyGetInfo"):
        assert name not in ffi.ENQUEUE_ONLY, name
    good = (0, 352, 96, 8)                      # (gpu, nstand, nfine, nsrc)
    for i, v in ((1, 0), (1, -3), (1, 513), (2, 0), (2, 65536), (3, -1), (3, 33)):
        args = list(good)
        args[i] = v
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCalapplyInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    s, b = ctypes.c_int(), ctypes.c_longlong()
    f64 = np.zeros(4, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    f32 = np.ones(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for name, args in (("xengCalapplyRun", (None, 4096)), ("xengCalapplyRun", (4096, None)), ("xengCalapplyRun", (4104, 4096)), ("xengCalapplyRun", (4096, 4104)),
                       ("xengCalapplyGetInfo", (None, ctypes.byref(s), ctypes.byref(s), ctypes.byref(b))),
                       ("xengCalapplyGetInfo", (ctypes.byref(s), None, ctypes.byref(s), ctypes.byref(b))),
                       ("xengCalapplyGetInfo", (ctypes.byref(s), ctypes.byref(s), None, ctypes.byref(b))),
                       ("xengCalapplyGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(s), None)),
                       ("xengCalapplySetModel", (f64, None, f32)), ("xengCalapplySetFactors", (None,)),
                       ("xengCalapplyMark", (None,)), ("xengCalapplyTicketDone", (1, None)), ("xengCalapplyCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_calapply_gpu.py covers the rest)
    t = ctypes.c_ulonglong()
    for name, args in (("xengCalapplyRun", (4096, 4096)), ("xengCalapplySetModel", (f64, f64, f32)), ("xengCalapplySetModel", (None, f64, None)),
                       ("xengCalapplySetFactors", (4096,)), ("xengCalapplyGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(s), ctypes.byref(b))),
                       ("xengCalapplyMark", (ctypes.byref(t),)), ("xengCalapplyWait", (1,)), ("xengCalapplyTicketDone", (1, ctypes.byref(s))),
                       ("xengCalapplySync", ()), ("xengCalapplyCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengCalapplyDestroy")     # (nothing to destroy: success)
