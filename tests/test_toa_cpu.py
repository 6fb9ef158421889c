"""BeamToa without a GPU: the host helpers (toa_subbands, toa_tables, toa_template, toa_refine, toa_dm_fit, toa_epoch), the
TOA_ENGINES row under the per-row checks of tests/test_engine_table_cpu.py, the C entry points' argument checks, the restatement
(tests/toa_ref.py) against the float64 statement (toa_reference) on integer data, and the block on CPU rings with a backend that
serves xengToa* by the restatement -- the header keys, the refusals, an inactive pair, the commands, and a planted pulsar whose
delay, DM error and arrival time come back within 5 Cramer-Rao errors computed from what was planted."""
import ctypes
import json
import threading
from fractions import Fraction

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi
from caltech_bifrost_dsp_amd.blocks import (TOA_RECORD, BeamToa, as_toa, subband_frequencies, toa_dm_fit, toa_epoch, toa_offsets, toa_reference, toa_refine,
                                            toa_subbands, toa_tables, toa_template)
from caltech_bifrost_dsp_amd.blocks.dedisp import KDM
from caltech_bifrost_dsp_amd.ring import Ring
from tests import test_engine_table_cpu, toa_cases, toa_ref
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, source_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2
_pf, _pb, _pi = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)


# ---------------------------------------------------------------- the host helpers
def test_subbands_offsets_and_views():
    assert toa_subbands(70, 3).tolist() == [0, 23, 46, 70] and toa_subbands(13, 13).tolist() == list(range(14)) and toa_subbands(5, 1).tolist() == [0, 5]
    assert toa_subbands(3072, 32).tolist() == list(range(0, 3073, 96)) and toa_subbands(70, 3).dtype == np.int32
    for bad in ((3, 4), (70, 0), (70, 257), (7.0, 2)):
        with pytest.raises(ValueError):
            toa_subbands(*bad)
    a, b, c, n = toa_offsets(2, 3, 100, 33, 257)
    assert (a, b, c, n) == (128, 128 + 3200, 128 + 3200 + 2112, 128 + 3200 + 2112 + 8224) and TOA_RECORD.itemsize == 16
    rec, P, PH, ccf = as_toa(np.zeros(n, np.uint8), 2, 3, 100, 33, 257)
    assert rec.shape == (2, 4) and P.shape == (2, 4, 100) and PH.shape == (2, 4, 33, 2) and ccf.shape == (2, 4, 257)
    with pytest.raises(ValueError):
        as_toa(np.zeros(n + 1, np.uint8), 2, 3, 100, 33, 257)


def test_tables_are_exact_at_the_quarter_turns_and_rounded_once():
    """k b = 0, nbin/4, nbin/2, 3 nbin/4 mod nbin give (1, 0), (0, -1), (-1, 0), (0, 1) exactly, with no -0; every other word is the
    float64 value of the integer-reduced argument rounded once (within half a float32 ulp of a longdouble evaluation)."""
    nbin, nharm, nlag = 64, 31, 100
    D, L = toa_tables(nbin, nharm, nlag)
    assert D.shape == (nbin, nharm, 2) and L.shape == (nharm, nlag, 2) and D.dtype == L.dtype == np.float32
    for T, n, rows in ((D, nbin, lambda b, k: (b, k - 1)), (L, nlag, lambda l, k: (k - 1, l))):
        for i in range(n):
            for k in range(1, nharm + 1):
                m = (k * i) % n
                v = T[rows(i, k)]
                if 4 * m % n == 0:
                    assert tuple(v.tolist()) == [(1.0, 0.0), (0.0, -1.0), (-1.0, 0.0), (0.0, 1.0)][4 * m // n] and not np.signbit(v[v == 0]).any(), (i, k)
        assert not np.signbit(T[T == 0]).any()
    ang = 2 * np.pi * np.longdouble(1) * ((np.arange(nbin)[:, None] * np.arange(1, nharm + 1)[None, :]) % nbin) / nbin
    want = np.stack([np.cos(ang), -np.sin(ang)], -1)
    assert np.all(np.abs(D.astype(np.longdouble) - want) <= 2.0 ** -24 * np.abs(want) + 1e-14)      # (half an ulp, and the float64 pi of this line)
    for bad in ((64, 32, 10), (64, 0, 10), (64, 31, 0), (64, 31, 65537), (16385, 4, 4), (2, 1, 1)):
        with pytest.raises(ValueError):
            toa_tables(*bad)


def test_template_is_a_float64_dft_with_the_band_row_the_sum_and_its_refusals():
    nbin, nharm = 40, 7
    prof = np.array([toa_cases.pulse(nbin, 11.3, 2.0), toa_cases.pulse(nbin, 3.0, 1.0)])
    S = toa_template(prof, nharm, nsub=3)
    assert S.shape == (2, 4, nharm, 2) and S.dtype == np.float32
    want = np.fft.fft(prof, axis=1)[:, 1:nharm + 1]
    for r in range(3):
        assert np.allclose(S[:, r, :, 0], want.real, rtol=1e-6, atol=1e-6) and np.allclose(S[:, r, :, 1], want.imag, rtol=1e-6, atol=1e-6)
    assert np.allclose(S[:, 3], 3 * np.stack([want.real, want.imag], -1), rtol=1e-6, atol=1e-6)
    per = np.stack([prof, 2 * prof, np.roll(prof, 1, axis=1)], axis=1)          # [npair][nsub][nbin]
    S3 = toa_template(per, nharm)
    assert S3.shape == (2, 4, nharm, 2) and np.allclose(S3[:, 3], S3[:, :3].astype(np.float64).sum(1), rtol=1e-6, atol=1e-6)
    for bad, kw in ((np.ones((2, nbin)), {}), (prof[:, :, None, None], {}), (np.where(np.arange(nbin) == 3, np.nan, prof), {}), (prof, dict(nsub=0))):
        with pytest.raises(ValueError):
            toa_template(bad, nharm, **kw)                                     # (a flat template has no power in the harmonics)
    with pytest.raises(ValueError, match="no power"):
        toa_template(np.stack([prof[0], np.cos(2 * np.pi * 9 * np.arange(nbin) / nbin)]), nharm)       # (power in harmonic 9 only)
    for nh in (0, 20):
        with pytest.raises(ValueError):
            toa_template(prof, nh)


def _harmonics(x, nharm):
    return np.stack([np.fft.fft(x)[1:nharm + 1].real, np.fft.fft(x)[1:nharm + 1].imag], -1)


@pytest.mark.parametrize("tau", [0.0, 0.3137, 0.9991, 0.5])
def test_refine_recovers_a_planted_fractional_shift(tau):
    """A band-limited template (harmonics 1..6) delayed by tau turns through a float64 Fourier shift, scaled by 3.5 on a baseline of
    2.  Noise-free: tau, found from the grid lag nearest to it, comes back to the float64 rounding of the scene (1e-12 turns; the
    harmonics are of order 10 and their phases are known to 1e-15) and b to 1e-12.  With seeded normal noise of 0.2 per bin: within
    5 Cramer-Rao errors, sigma_F / (b sqrt(2 sum k^2 |S_k|^2)) / 2 pi with sigma_F^2 = nbin sigma^2 / 2, computed here from what was
    planted; toa_refine's own tau_err (from the off-pulse variance handed in) agrees with it, and the reduced chi^2 is near 1."""
    nbin, nharm, nlag, amp = 64, 6, 256, 3.5
    k = np.arange(1, nharm + 1)
    a = 1.0 / k
    x = np.arange(nbin) / nbin

    def shape(t):
        return np.sum(a[:, None] * np.cos(2 * np.pi * k[:, None] * (x[None, :] - 0.2 - t)), 0)
    S = _harmonics(shape(0.0), nharm)
    clean = 2.0 + amp * shape(tau)
    l = int(round(tau * nlag)) % nlag
    tau_l = tau - 1 if tau > 0.99 else tau                     # (0.9991 is found next to lag 0, as -0.0009)
    f = toa_refine(_harmonics(clean, nharm), S, l, nlag, 1.0, nbin)
    assert f['bracketed'] and abs(f['tau'] - tau_l) < 1e-12 and abs(f['b'] - amp) < 1e-12
    if tau == 0.3137:           # lag 81 instead of 80: the root (80.3 lags) is still inside the bracket; from lag 82 it is not
        assert abs(toa_refine(_harmonics(clean, nharm), S, l + 1, nlag, 1.0, nbin)['tau'] - tau) < 1e-12
        far = toa_refine(_harmonics(clean, nharm), S, l + 2, nlag, 1.0, nbin)
        assert not far['bracketed'] and far['tau'] == (l + 2) / nlag
    sigma = 0.2
    cr = toa_cases.cramer_rao(S, amp, sigma, nbin)
    worst = 0.0
    for seed in range(8):
        noisy = clean + sigma * np.random.default_rng(100 + seed).standard_normal(nbin)
        PH = _harmonics(noisy, nharm)
        ccf = np.array([np.sum(((PH[:, 0] + 1j * PH[:, 1]) * np.conj(S[:, 0] + 1j * S[:, 1]) * np.exp(2j * np.pi * k * i / nlag)).real) for i in range(nlag)])
        f = toa_refine(PH, S, int(ccf.argmax()), nlag, sigma ** 2, nbin)
        err = (f['tau'] - tau + 0.5) % 1 - 0.5
        worst = max(worst, abs(err) / cr)
        assert f['bracketed'] and abs(err) <= 5 * cr and abs(f['b'] - amp) <= 5 * f['b_err']
        assert 0.9 < f['tau_err'] / cr < 1.1 and 0.2 < f['chi2'] < 3.0 and abs(f['snr'] - f['b'] / f['b_err']) < 1e-9
    print("toa_refine: Cramer-Rao error %.3g turns, worst |error| / CR = %.2f" % (cr, worst))
    assert toa_refine(_harmonics(clean, nharm), S, -1, nlag, 1.0, nbin) is None
    assert toa_refine(np.full((nharm, 2), np.nan), S, 0, nlag, 1.0, nbin) is None


def test_dm_fit_recovers_a_planted_dm_error_unwraps_and_needs_two_sub_bands():
    f0, ddm, tau_inf = 3.7, 0.004, 0.31
    freqs = np.array([62e6, 67e6, 72e6, 77e6])
    x = KDM * f0 * (freqs * 1e-6) ** -2
    sig = np.array([2e-3, 1.5e-3, 1e-3, 1e-3])
    for seed in range(6):
        tau = tau_inf + ddm * x + sig * np.random.default_rng(seed).standard_normal(4)
        wrapped = tau - np.floor(tau)                       # (what a correlation gives: a fraction of a turn)
        d = toa_dm_fit(wrapped, sig, freqs, f0, tau_band=float(np.mean(tau)))
        assert abs(d['dm'] - ddm) <= 5 * d['dm_err'] and abs(d['tau_inf'] - tau_inf) <= 5 * d['tau_inf_err'] and d['nused'] == 4 and d['chi2'] < 20
        assert np.allclose(d['tau'], tau, atol=1e-12)
    de, te = toa_cases.line_errors(sig, x, 0.0)
    assert abs(d['dm_err'] - de) < 1e-12 * de + 1e-18 and abs(d['tau_inf_err'] - te) < 1e-9 * te
    exact = toa_dm_fit(tau_inf + ddm * x, sig, freqs, f0)
    assert abs(exact['dm'] - ddm) < 1e-12 and abs(exact['tau_inf'] - tau_inf) < 1e-9 and exact['chi2'] < 1e-12
    one = toa_dm_fit([0.3, None, np.nan, 0.2], [1e-3, 1e-3, 1e-3, np.inf], freqs, f0)
    assert one['dm'] is None and one['tau_inf'] is None and one['nused'] == 1
    assert toa_dm_fit([0.3], [1e-3], freqs[:1], f0)['dm'] is None and toa_dm_fit([None], [None], freqs[:1], f0)['nused'] == 0
    with pytest.raises(ValueError):
        toa_dm_fit([0.1, 0.2], [1e-3, 1e-3], [60e6, -1.0], f0)
    fr = subband_frequencies(np.array([60e6, 70e6, 80e6, 90e6]), [0, 2, 2, 4], [1, 1, 0, 0])
    assert abs(fr[0] - ((60e6 ** -2 + 70e6 ** -2) / 2) ** -0.5) < 1e-3 and np.isnan(fr[1]) and np.isnan(fr[2])


@pytest.mark.parametrize("f1,pepoch", [(0.0, 0.0), (0.0, 1.25), (-3.0e-4, 0.75)])
def test_epoch_agrees_with_a_rational_evaluation_of_the_phase_model(f1, pepoch):
    """The time returned has the model phase N + tau + 1/(2 nbin) for an integer N -- exactly where f1 = 0, to 1e-30 turns else --
    and no other such time lies nearer the sub-integration's midpoint."""
    hdr = dict(nchan=3, bw_hz=19.6e6, subint_start=4096 * 32, subint_nwindow=64, tsamp=32 * 3 / 19.6e6, nbin=16,
               pulsars=[None, dict(f0=12755.1, f1=f1, pepoch=pepoch, dm=1.0)])
    f0, f1q, pe = Fraction(12755.1), Fraction(f1), Fraction(pepoch)
    t_mid = Fraction(4096 * 32) * Fraction(3) / Fraction(19.6e6) + 64 * Fraction(32 * 3 / 19.6e6) / 2
    for tau in (0.0, 0.2371, -0.004, 0.999):
        t = toa_epoch(hdr, 1, tau)
        assert isinstance(t, Fraction)
        phi = f0 * (t - pe) + f1q * (t - pe) ** 2 / 2
        frac = phi - Fraction(float(tau)) - Fraction(1, 32)
        assert abs(frac - round(frac)) <= (0 if f1 == 0 else Fraction(1, 10 ** 30))
        f_now = f0 + f1q * (t_mid - pe)
        assert abs(t - t_mid) <= Fraction(1, 2) / f_now * (1 + Fraction(1, 10 ** 6))
    with pytest.raises(ValueError):
        toa_epoch(hdr, 0, 0.1)


# ---------------------------------------------------------------- the engine's row and the entry points
def test_the_new_row_passes_the_symbol_checks_of_the_engine_table():
    assert ffi.TOA_ENGINES == [("Toa", "toa", True)] and ffi.RMSYNTH_ENGINES == [("Rmsynth", "rmsynth", True)]
    older = ffi.ENGINES + ffi.MORE_ENGINES + ffi.NEWER_ENGINES + ffi.NEWEST_ENGINES + ffi.LATEST_ENGINES + ffi.FURTHER_ENGINES + ffi.CUTOUT_ENGINES + \
        ffi.RMSYNTH_ENGINES
    assert not {r[0] for r in ffi.TOA_ENGINES} & {r[0] for r in older} and not {r[1] for r in ffi.TOA_ENGINES} & {r[1] for r in older}
    assert len(ffi.ENQUEUE_ONLY) == len(set(ffi.ENQUEUE_ONLY))
    for row in ffi.TOA_ENGINES:
        test_engine_table_cpu.test_symbols_and_methods_of_a_row(*row)


def test_the_new_row_keeps_the_status_contract_without_a_gpu():
    for row in ffi.TOA_ENGINES:
        test_engine_table_cpu.test_status_contract_of_a_row_without_a_gpu(*row)


def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    L = ffi.lib()
    counts = dict(Initialize=8, SetBands=2, SetTables=2, SetTemplate=1, SetMask=1, SetActive=1, Run=2, Reset=0, GetInfo=6, CheckGuards=1, Mark=1, Wait=1,
                  TicketDone=2, Sync=0, Destroy=0)
    for n, argc in counts.items():
        name = "xengToa" + n
        assert hasattr(L, name) and name in test_engine_table_cpu.DECLARED and len(ffi.SYMBOLS[name]) == argc, name
        assert (name in ffi.ENQUEUE_ONLY) == (n in ("Run", "Reset", "Mark", "TicketDone")), name
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("initialize", "set_bands", "set_tables", "set_template", "set_mask", "set_active", "run", "reset", "info", "guards_intact", "mark", "wait",
              "ticket_done", "sync"):
        assert callable(getattr(HipBackend, "toa_" + m)), m
    good = [2, 1, 8, 16, 2, 4, 32]                                  # (npair, nprod, nchg, nbin, nsub, nharm, nlag)
    for i, v in ((0, 0), (0, 65536), (1, 0), (1, 2), (1, 3), (2, 0), (2, 65537), (3, 0), (3, 16385), (4, 0), (4, 257), (5, 0), (5, 8), (6, 0), (6, 65537)):
        args = list(good)
        args[i] = v
        assert L.xengToaInitialize(0, *args) == INVALID_ARGUMENT, args
    assert L.xengToaInitialize(0, 1, 1, 8, 16384, 1, 4097, 16) == INVALID_ARGUMENT                                         # (nharm above 4096)
    assert L.xengToaInitialize(0, 1, 1, 8, 16384, 1, 4096, 65536) == INVALID_ARGUMENT and b"table" in L.xengGetLastError()      # 2 GiB of lags
    assert L.xengToaInitialize(0, 65535, 1, 8, 16384, 256, 4, 16) == INVALID_ARGUMENT and b"4 GiB" in L.xengGetLastError()
    if not _gpu_present():
        assert L.xengToaInitialize(0, *good) not in (0, INVALID_ARGUMENT)              # (good sizes get as far as the device)
    for a, b in ((None, 16), (16, None), (20, 16), (16, 24)):
        assert L.xengToaRun(a, b) == INVALID_ARGUMENT
    assert L.xengToaGetInfo(None, None, None, None, None, None) == INVALID_ARGUMENT and L.xengToaSetBands(None, None) == INVALID_ARGUMENT
    assert L.xengToaSetTables(None, None) == INVALID_ARGUMENT and L.xengToaSetTemplate(None) == INVALID_ARGUMENT
    if not _gpu_present():
        n, k = ctypes.c_longlong(), (ctypes.c_int * 4)()
        T = np.zeros((64, 2), np.float32)
        e = np.zeros(3, np.int32)
        assert L.xengToaRun(16, 16) == INVALID_STATE and L.xengToaReset() == INVALID_STATE
        assert L.xengToaSetBands(e.ctypes.data_as(_pi), None) == INVALID_STATE and L.xengToaSetTables(T.ctypes.data_as(_pf), T.ctypes.data_as(_pf)) == INVALID_STATE
        assert L.xengToaSetTemplate(T.ctypes.data_as(_pf)) == INVALID_STATE and L.xengToaSetMask(None) == INVALID_STATE and L.xengToaSetActive(None) == INVALID_STATE
        assert L.xengToaGetInfo(ctypes.byref(n), k, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == INVALID_STATE


# ---------------------------------------------------------------- the restatement against the float64 statement
@pytest.mark.parametrize("nprod", [1, 4])
def test_on_integer_data_the_restatement_equals_the_float64_statement_exactly(nprod):
    """Integers 0..1 in 2 pairs x 13 groups x 20 bins, weights of 0 and 1, 16 off-pulse bins (the baseline is a multiple of 1/16),
    tables of -1, 0, 1 in D and S and the l = 0 column of the lag table alone (L = (1, 0)): every float32 step is exact (every sum an
    integer multiple of 1/256 below 2^24), so P, base, var, PH and ccf equal toa_reference's float64 values word for word."""
    c = integer_case(nprod)
    rec, P, PH, ccf = toa_ref.toa(c['X'], c['edges'], c['w'], c['D'], c['L'], c['S'], c['off'])
    e = toa_reference(np.where(np.isfinite(c['X']), c['X'], 0), c['edges'], c['w'], c['D'], c['L'], c['S'], c['off'])
    for got, want in ((P, e['P']), (rec['base'], e['base']), (rec['var'], e['var']), (PH, e['PH']), (ccf, e['ccf'])):
        assert np.array_equal(got.astype(np.float64), want)
    assert rec['l'].tolist() == e['l'].tolist() and set(rec['l'].ravel().tolist()) == {0} and np.array_equal(rec['peak'], ccf[:, :, 0])
    assert PH.any() and ccf.any() and np.abs(e['ccf']).max() * 256 < 2 ** 24


def integer_case(nprod):
    rng = np.random.default_rng(40 + nprod)
    edges = np.array([0, 4, 8, 13], np.int32)
    w = np.ones(13, np.float32)
    w[[5, 11]] = 0
    off = np.zeros((2, 20), np.uint8)
    off[0, :16], off[1, 2:18] = 1, 1
    X = toa_cases.poison_unused(toa_cases.integer_scene(7 + nprod, 2, nprod, 13, 20, top=2), edges, w)
    return dict(X=X, edges=edges, w=w, D=rng.integers(-1, 2, (20, 4, 2)).astype(np.float32), L=np.tile(np.array([1, 0], np.float32), (4, 1, 1)),
                S=rng.integers(-1, 2, (2, 4, 4, 2)).astype(np.float32), off=off)


# ---------------------------------------------------------------- the block on CPU rings
class ToaBackend(OracleBackend):
    """The oracle backend plus xengToa* served by the restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.k, self.calls, self.bands, self.tables, self.S, self.off, self.active = None, [], None, None, None, None, None

    def toa_initialize(self, gpu, npair, nprod, nchg, nbin, nsub, nharm, nlag):
        self.k = dict(npair=npair, nprod=nprod, nchg=nchg, nbin=nbin, nsub=nsub, nharm=nharm, nlag=nlag)
        self.calls.append(('init', npair, nprod, nchg, nbin, nsub, nharm, nlag))
        return 0

    def toa_set_bands(self, edges, w=None):
        assert edges.dtype == np.int32 and edges.shape == (self.k['nsub'] + 1,) and (w is None or (w.dtype == np.float32 and w.shape == (self.k['nchg'],)))
        self.bands = (edges.copy(), None if w is None else w.copy())
        self.calls.append('set_bands')
        return 0

    def toa_set_tables(self, D, L):
        k = self.k
        assert D.dtype == L.dtype == np.float32 and D.shape == (k['nbin'], k['nharm'], 2) and L.shape == (k['nharm'], k['nlag'], 2)
        self.tables = (D.copy(), L.copy())
        self.calls.append('set_tables')
        return 0

    def toa_set_template(self, S):
        k = self.k
        assert S.dtype == np.float32 and S.shape == (k['npair'], k['nsub'] + 1, k['nharm'], 2) and S.flags.c_contiguous
        self.S = S.copy()
        self.calls.append('set_template')
        return 0

    def toa_set_mask(self, off=None):
        assert off is None or (off.dtype == np.uint8 and off.shape == (self.k['npair'], self.k['nbin']))
        self.off = off
        self.calls.append('set_mask')
        return 0

    def toa_set_active(self, active=None):
        self.active = None if active is None else active.copy()
        self.calls.append(('set_active', None if active is None else active.tolist()))
        return 0

    def toa_run(self, in_arr, out_arr):
        k = self.k
        X = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape(k['npair'], k['nprod'], k['nchg'], k['nbin'])
        out = toa_ref.out_bytes(*toa_ref.toa(X, self.bands[0], self.bands[1], *self.tables, self.S, self.off, self.active))
        out_arr.numpy().reshape(-1).view(np.uint8)[...] = out
        self.calls.append('run')
        return 0

    def toa_reset(self):
        self.calls.append('reset')

    def toa_mark(self):
        return self.beam_mark()

    def toa_wait(self, ticket):
        self.beam_wait(ticket)

    def toa_sync(self):
        pass


NPAIR, NCHAN, NUP, NBIN, NSUB, NHARM, NLAG, NWINDOW = 2, 3, 32, 16, 4, 5, 64, 64
NFINE = NCHAN * NUP
TSAMP = NUP * NCHAN / 19.6e6
F0 = 1.0 / (NBIN * TSAMP)
FREQS = 60e6 + 19.6e6 / NFINE * np.arange(NFINE)
PSR = dict(f0=F0, f1=0.0, pepoch=0.0, dm=0.0)
TAUS, DDM, NOISE = (0.2371, 0.61), 1e-5, 0.3
TEMPLATE = np.array([toa_cases.planted_template(NBIN)] * NPAIR)
OFF = np.ones((NPAIR, NBIN), np.uint8)


def fold_header(seq0=0, nprod=1, **extra):
    """The sequence header BeamFold(nfscr=1) writes (beam_fold_block.py output_header) over 60 to 79.6 MHz."""
    chan_bw = 19.6e6 / NCHAN
    hdr = source_header(NCHAN, NPAIR, 2, seq0=seq0, sfreq=60e6, chan_bw=chan_bw)
    hdr.update(nstand=NPAIR, nbeam=NPAIR, npol=2, complex=True, nbit=32, nupchan=NUP, nframe_sum=1, fine_bw_hz=chan_bw / NUP, fine_sfreq=60e6, pair0=0,
               acc_len=NUP, nbin=NBIN, nfscr=1, nprod=nprod, tsamp=TSAMP, nsub=4, pulsars=[PSR, PSR], normalise=True, hits=[[4] * NBIN] * NPAIR,
               subint_start=seq0, subint_nwindow=NWINDOW)
    hdr.update(extra)
    return hdr


def _block(seqs, be=None, **kw):
    be = be or ToaBackend()
    r1 = Ring("toa-output")
    fake = _FakeRing([_FakeSeq(h, [(0, x)], x.nbytes) for h, x in seqs])
    blk = BeamToa(LOG, fake, r1, backend=be, **dict(dict(npair=NPAIR, nchg=NFINE, nbin=NBIN, nsub=NSUB, templates=TEMPLATE, nharm=NHARM, nlag=NLAG), **kw))
    return blk, be, Sink(r1, toa_offsets(NPAIR, NSUB, NBIN, NHARM, NLAG)[3])


def planted_errors(off):
    """(the Cramer-Rao errors of tau at the reference frequency and of the DM offset, x_ref) for the planted pulsar: sub-bands of 24
    channels whose folded bins hold the mean of 4 windows of XX + YY (noise NOISE sqrt(2) / 2 per channel and bin), fitted by a line."""
    S = toa_template(TEMPLATE, NHARM, NSUB).astype(np.float64)
    edges = toa_subbands(NFINE, NSUB)
    fr = subband_frequencies(FREQS, edges)
    cr = [toa_cases.cramer_rao(S[0, r], 1.0, NOISE * np.sqrt(2.0) / 2 * np.sqrt(24.0) / 24.0, NBIN) for r in range(NSUB)]
    x_ref = KDM * F0 * (FREQS.max() * 1e-6) ** -2
    return toa_cases.line_errors(cr, KDM * F0 * (fr * 1e-6) ** -2, x_ref)[::-1] + (x_ref,)


def check_planted(toas, hdr, tau_err, dm_err, taus=TAUS):
    """The header's toas of one sub-integration against what was planted, within 5 of the errors given."""
    worst = 0.0
    for p, t in enumerate(toas):
        if t is None:
            continue
        dt = (t['tau'] - taus[p] + 0.5) % 1 - 0.5
        t_mid = (hdr['subint_start'] * NCHAN / 19.6e6) + hdr['subint_nwindow'] * TSAMP / 2
        n = round(F0 * t_mid - taus[p] - 0.5 / NBIN)
        planted = (n + taus[p] + 0.5 / NBIN) / F0                                   # (f1 = 0, pepoch = 0)
        worst = max(worst, abs(dt) / tau_err, abs(t['dm_offset'] - DDM) / dm_err, abs(float(t['toa_s']) - planted) * F0 / tau_err)
        assert abs(dt) <= 5 * tau_err and abs(t['dm_offset'] - DDM) <= 5 * dm_err and abs(float(t['toa_s']) - planted) <= 5 * tau_err / F0, (p, t)
        assert t['snr'] > 5 and t['dm_err'] > 0 and t['tau_err'] > 0       # (5.6 where every bin counts as off-pulse: the pulse is in the variance)
    return worst


def test_block_measures_a_planted_pulsar_with_the_header_keys_an_inactive_pair_and_commands():
    """Four sub-integrations of 64 windows of the planted pulsar (delays 0.2371 and 0.61 turns, a DM error of 1e-5, noise 0.3) folded
    in float64, nprod 1, 1, 4, 4 (the context is made again for the other nprod).  The first with both pairs; the second's header
    has no pulsar for pair 1 (inactive: -1 and +0, toas None); before the third a `masks` command (off = the bins away from the
    pulses) and a `weights` command that leaves group 30 out; before the fourth a `templates` command (the templates moved by one
    bin: tau comes back one bin smaller).  Every span equals the restatement byte for byte, and tau, dm_offset and toa_s agree with
    what was planted within 5 Cramer-Rao errors."""
    x = [toa_cases.planted_windows(50 + i, NWINDOW, NPAIR, FREQS, NBIN, F0, TAUS, DDM, noise=NOISE) for i in range(4)]
    nprods = [1, 1, 4, 4]
    cubes = [toa_cases.fold_cube(xi, NBIN, n) for xi, n in zip(x, nprods)]
    starts = [0, 64 * NUP, 128 * NUP, 192 * NUP]
    hdrs = [fold_header(starts[0]), fold_header(starts[1], pulsars=[PSR, None]), fold_header(starts[2], nprod=4), fold_header(starts[3], nprod=4)]
    off = np.ones((NPAIR, NBIN), np.uint8)
    for p in range(NPAIR):
        c = int(round((TAUS[p] + 0.03) * NBIN))
        off[p, [(c + d) % NBIN for d in range(-4, 5)]] = 0
    wnew = np.ones(NFINE)
    wnew[30] = 0
    moved = np.roll(TEMPLATE, 1, axis=1)
    blk, be, sink = _block(list(zip(hdrs, cubes)))
    seen = []

    def on_span(hdr, n):
        seen.append(hdr['seq0'])
        if hdr['seq0'] == starts[1]:
            blk.process_command_strings(json.dumps({'cmd': 'update', 'id': '1', 'val': {'kwargs': {'masks': dict(off=off.tolist()), 'weights': wnew.tolist()}}}))
        if hdr['seq0'] == starts[2]:
            blk.process_command_strings(json.dumps({'cmd': 'update', 'id': '2', 'val': {'kwargs': {'templates': moved.tolist()}}}))
        gate.set()
    gate = threading.Event()
    sink.on_span = on_span
    # (the fake input ring hands the sequences over at once: run the block from the sink's side span by span)
    orig = blk._check_header
    first = [True]

    def stepped(ihdr):
        if not first[0]:
            assert gate.wait(20)
            gate.clear()
        first[0] = False
        orig(ihdr)
    blk._check_header = stepped
    sink.start()
    blk.main()
    sink.join(20)
    assert seen == starts and len(sink.sequences) == 4 and all(len(s[2]) == 1 for s in sink.sequences)
    edges = toa_subbands(NFINE, NSUB)
    D, L = toa_tables(NBIN, NHARM, NLAG)
    S0, S1 = toa_template(TEMPLATE, NHARM, NSUB), toa_template(moved, NHARM, NSUB)
    a, b, c, n = toa_offsets(NPAIR, NSUB, NBIN, NHARM, NLAG)
    tau_err, dm_err, _ = planted_errors(None)
    wf = wnew.astype(np.float32)
    want = [(None, S0, None, None), (None, S0, None, np.array([1, 0], np.uint8)), (wf, S0, off, None), (wf, S1, off, None)]
    for i, ((hd, tag, spans), h, cube, (w, S, o, act)) in enumerate(zip(sink.sequences, hdrs, cubes, want)):
        assert tag == h['seq0'] and (hd['toa_nsub'], hd['toa_nharm'], hd['toa_nlag'], hd['toa_edges']) == (NSUB, NHARM, NLAG, edges.tolist())
        assert (hd['record_offset'], hd['profile_offset'], hd['harmonic_offset'], hd['ccf_offset'], hd['span_bytes']) == (0, a, b, c, n)
        assert hd['nbin'] == NBIN and hd['nprod'] == nprods[i] and np.allclose(hd['toa_freqs'], subband_frequencies(FREQS, edges, w))
        exp = toa_ref.out_bytes(*toa_ref.toa(cube, edges, w, D, L, S, o, act))
        assert spans[0].tobytes() == exp.tobytes()
        rec, P, PH, ccf = as_toa(spans[0], NPAIR, NSUB, NBIN, NHARM, NLAG)
        assert (rec[0]['l'] >= 0).all() and set(hd['toas'][0]) == {'tau', 'tau_err', 'toa_s', 'dm_offset', 'dm_err', 'snr', 'chi2'}
        if act is not None:
            assert hd['toas'][1] is None and all(r.tolist() == (-1, 0.0, 0.0, 0.0) for r in rec[1]) and not P[1].any() and not ccf[1].any()
        taus = TAUS if i < 3 else tuple(t - 1.0 / NBIN for t in TAUS)
        worst = check_planted(hd['toas'], hd, tau_err, dm_err, taus)
        print("sub-integration %d: worst error / Cramer-Rao = %.2f (tau_err %.3g turns, dm_err %.3g)" % (i, worst, tau_err, dm_err))
        if o is not None:       # (with a real off-pulse mask the block's own errors are of the Cramer-Rao ones' size and chi^2 of order 1:
            # the variance comes from 7 off-pulse bins, a chi^2 of 7 degrees of freedom, so within a factor of a few)
            assert all(0.3 < t['dm_err'] / dm_err < 2 and 0.1 < t['chi2'] < 10 for t in hd['toas'])
    assert be.calls[0] == ('init', NPAIR, 1, NFINE, NBIN, NSUB, NHARM, NLAG) and [c for c in be.calls if c[0] == 'init'][1][2] == 4
    assert be.calls.count('run') == 4 and be.calls.count('set_tables') == 2 and be.calls.count('set_template') == 3 and be.calls.count('set_bands') == 3
    assert [c for c in be.calls if isinstance(c, tuple) and c[0] == 'set_active'] == [('set_active', [1, 1]), ('set_active', [1, 0]), ('set_active', [1, 1])]
    assert blk.stats['nsubint'] == 4 and blk.stats['ntoa'] == 7 and json.dumps(sink.sequences[0][0])


@pytest.mark.parametrize("change,msg", [(dict(nbin=None), "nbin"), (dict(nprod=2), "nprod"), (dict(rm_phis=[0.0]), "rm_phis"), (dict(toa_nlag=64), "toa_nlag"),
                                        (dict(nbin=32), "bins"), (dict(nfscr=2), "groups"), (dict(nbeam=3), "pairs"), (dict(fine_bw_hz=0.0), "fine_bw_hz")])
def test_block_refuses_what_is_not_a_folded_cube(change, msg):
    hdr = fold_header()
    for k, v in change.items():
        if v is None:
            del hdr[k]
        else:
            hdr[k] = v
    blk, be, _ = _block([(hdr, np.zeros((NPAIR, 1, NFINE, NBIN), np.float32))])
    with pytest.raises(ValueError, match=msg):
        blk.main()
    assert 'run' not in be.calls


@pytest.mark.parametrize("kw", [dict(npair=0), dict(nchg=0), dict(nbin=16385), dict(nbin=2), dict(nchg=96.0), dict(nsub=0), dict(nsub=97), dict(nharm=8), dict(nharm=0),
                                dict(nlag=0), dict(nlag=65537), dict(templates=np.ones((NPAIR, NBIN))), dict(templates=TEMPLATE[:1]),
                                dict(templates=np.zeros((NPAIR, 3, NBIN))), dict(weights=[1.0]), dict(weights=[0.0] * NFINE),
                                dict(off=np.ones((NPAIR, NBIN + 1), np.uint8)), dict(off=np.full((NPAIR, NBIN), 2, np.uint8))])
def test_constructor_refuses_bad_arguments(kw):
    be = ToaBackend()
    with pytest.raises(ValueError, match="BEAM_TOA"):
        BeamToa(LOG, Ring("a"), Ring("b"), backend=be, **dict(dict(npair=NPAIR, nchg=NFINE, nbin=NBIN, nsub=NSUB, templates=TEMPLATE, nharm=NHARM, nlag=NLAG), **kw))
    assert be.k is None
