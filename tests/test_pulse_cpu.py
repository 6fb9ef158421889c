"""BeamPulseSearch without a GPU, both ring implementations: the restatement (tests/pulse_ref.py) against a term-by-term loop and
on planted box pulses of every width; pulse_candidates on hand-built planes (runs, ties, an empty plane, a threshold at exactly
a value); the block on CPU rings with a backend that keeps the context's state (the windows since the reset) and serves
xengPulse* by the float32 restatement -- spans within and across sequences, the output header, a gap (reset, a new output
sequence), a threshold command landing at the next span, the `sample` arithmetic against a pulse planted at a known sample,
refusals -- and the C entry points' argument checks."""
import ctypes
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import BeamPulseSearch, pulse_candidates
from caltech_bifrost_dsp_amd.blocks.pulse_search import RECORD, as_records
from caltech_bifrost_dsp_amd.ring import Ring
from tests.fake_backend import OracleBackend
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.pulse_ref import merge_records, pulse_search, pulse_search_naive, series
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
DMS = [0.0, 0.5, 1.0, 1.5, 2.0]


@pytest.fixture(params=["native", "python"], autouse=True)
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


def dedisp_header(npair, ndm, nprod, seq0=0, S=5, acc_len=32, **extra):
    """The sequence header BeamDedisperse writes (beam_dedisperse_block.py output_header) on UpchanSumBeams' header."""
    nchan, N = 2, 8
    hdr = source_header(nchan, npair, 2, seq0=seq0, sfreq=20e6)
    hdr.update(nstand=npair, nbeam=npair, npol=2, complex=True, nbit=32, nupchan=N, nframe_sum=acc_len // N, acc_len=acc_len,
               ndm=ndm, dms=[float(d) for d in np.arange(ndm) * 0.5], dedisp_latency=S, nprod=nprod, tsamp=acc_len * nchan / hdr['bw_hz'])
    hdr.update(extra)
    return hdr


def plane_of(rec):
    """A pulse_ref record (dict of arrays [npair][ndm]) as the plane the library writes."""
    out = np.zeros(rec['n'].shape, RECORD)
    out['snr'], out['n'], out['iw'], out['B'] = rec['snr'], rec['n'], rec['iw'], rec['B']
    return out


class PulseBackend(OracleBackend):
    """The oracle backend plus xengPulse* served by the float32 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.ps, self.calls = None, []

    def pulse_initialize(self, gpu, npair, ndm, nwin, nprod, nwidth, nstat):
        self.ps = dict(npair=npair, ndm=ndm, nwin=nwin, nprod=nprod, nwidth=nwidth, nstat=nstat)
        self.x = []
        self.calls.append(('init', nprod))
        return 0

    def pulse_run(self, in_arr, nwin_call, out_arr):
        u = self.ps
        assert 1 <= nwin_call <= u['nwin']
        x = in_arr.numpy().reshape(-1).view(np.uint8).view(np.float32).reshape(nwin_call, u['npair'], u['ndm'], u['nprod'])
        self.x.append(x.copy())
        z = series(np.concatenate(self.x), np.float32)
        rec = pulse_search(z, u['nstat'], u['nwidth'], np.float32, [a.shape[0] for a in self.x])['records'][-1]
        out_arr.numpy().reshape(-1).view(np.uint8)[...] = plane_of(rec).reshape(-1).view(np.uint8)
        self.calls.append('run')
        return 0

    def pulse_reset(self):
        self.x = []
        self.calls.append('reset')

    def pulse_mark(self):
        return self.beam_mark()

    def pulse_wait(self, ticket):
        self.beam_wait(ticket)

    def pulse_sync(self):
        pass


def _noise(rng, nwindows, npair, ndm, nprod):
    return rng.integers(0, 50, (nwindows, npair, ndm, nprod)).astype(np.float32)


def _cmd(threshold, seq_id="1"):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': {'threshold': threshold}}})


# ---------------------------------------------------------------- the restatement
def test_restatement_is_the_definition():
    """Against one term at a time, in float64: float data with a mean far above sigma, a constant series (v = 0), a NaN and an
    Inf window, calls of uneven sizes that cut blocks and boxcars; and the float32 restatement equals the float64 one on integer
    data wherever nothing rounds (c, m, v, B)."""
    rng = np.random.default_rng(3)
    nwindows, nser, nstat, nwidth = 45, 6, 6, 3
    z = 60 + rng.standard_normal((nwindows, nser))
    z[:, 1] = 7.0
    z[20, 2] = np.nan
    z[27, 3] = np.inf
    sizes = [1, 7, 5, 12, 3, 17]
    ref = pulse_search(z, nstat, nwidth, np.float64, sizes)
    snr, scored, recs = pulse_search_naive(z, nstat, nwidth, sizes)
    assert np.array_equal(ref['scored'], scored)
    assert scored[:nstat].sum() == 0 and not scored[:, :, 1].any() and scored[nstat:, 0, 0].all()
    assert not scored[nstat + 1, 2, 0] and scored[nstat + 3, 2, 0]                 # (a boxcar of 4 must begin at nstat or later)
    assert not scored[20:23, 2, 2].any() and not scored[24:30, :, 2].any() and scored[30, 0, 2] and not scored[32, 2, 2] and scored[33, 2, 2]
    assert scored[27, 0, 3] and np.isposinf(ref['snr'][27, 0, 3]) and not scored[30:36, :, 3].any() and scored[36, 0, 3]
    both = np.isfinite(snr) & scored
    assert np.allclose(ref['snr'][both], snr[both], rtol=1e-9, atol=1e-9)
    for k, per in enumerate(recs):
        for s, (v, n, iw, B) in enumerate(per):
            got = ref['records'][k]
            assert (got['n'][s], got['iw'][s]) == (n, iw), (k, s)
            if n >= 0 and np.isfinite(v):
                assert abs(got['snr'][s] - v) <= 1e-9 * max(1, abs(v)) and abs(got['B'][s] - B) <= 1e-9 * max(1, abs(B))
    assert [r['n'][1] for r in ref['records']] == [-1] * len(sizes) and ref['records'][0]['snr'][0] == 0
    zi = rng.integers(0, 50, (nwindows, nser)).astype(np.float32)
    a, b = pulse_search(zi, 8, nwidth, np.float64, sizes), pulse_search(zi, 8, nwidth, np.float32, sizes)
    for f in ('c', 'm', 'v', 'B'):
        assert b[f].dtype == np.float32 and np.array_equal(a[f], b[f].astype(np.float64), equal_nan=True), f
    assert np.array_equal(a['scored'], b['scored'])


@pytest.mark.parametrize("iw", range(8))
def test_restatement_recovers_a_planted_box_pulse(iw):
    """Noise of sigma 1 on a mean of 60, nstat = 128; a box of w = 2^iw windows, 100 sigma / sqrt(w) each, ending at the last
    window n1 of block 2 (so that the block before it, which normalises it, is free of the pulse): the best record of the run is
    (n1, iw) -- one window earlier the box loses 100 / w against a noise step of sqrt(2 / w), six sigma at w = 128 -- and its
    score is 100 within the error of a sigma estimated from 128 windows, in whichever call n1 falls."""
    rng = np.random.default_rng(10 + iw)
    nstat, nwidth, w, n1 = 128, 8, 1 << iw, 383
    z = 60 + rng.standard_normal((512, 3))
    z[n1 - w + 1:n1 + 1, 1] += 100 / np.sqrt(w)
    sizes = [30] * 17 + [2]
    ref = pulse_search(z, nstat, nwidth, np.float64, sizes)
    best = merge_records(ref['records'], sizes)
    assert (best['n'][1], best['iw'][1]) == (n1, iw) and abs(best['snr'][1] - 100) < 25
    assert best['snr'][0] < 7 and best['snr'][2] < 7
    k = n1 // 30
    assert ref['records'][k]['n'][1] == n1 - 30 * k and ref['records'][k]['iw'][1] == iw


# ---------------------------------------------------------------- pulse_candidates
def _plane(npair, ndm):
    p = np.zeros((npair, ndm), RECORD)
    p['n'], p['iw'] = -1, -1
    return p


def test_pulse_candidates_runs_ties_empty_and_threshold():
    dms = np.arange(8) * 0.5
    widths = [1, 2, 4, 8]
    p = _plane(2, 8)
    assert pulse_candidates(p, 8.0, dms, widths) == []
    assert pulse_candidates(p, -1.0, dms, widths) == []                         # (nothing scored: not a candidate at any threshold)
    # pair 0: trials 1-3 form a run (peak at 2), trial 5 another, trial 7 sits exactly at the threshold; pair 1: a tie over 4, 5
    for d, (snr, n, iw) in {1: (8.5, 3, 0), 2: (11.0, 4, 2), 3: (9.0, 4, 1), 5: (8.25, 0, 3), 7: (8.0, 2, 0)}.items():
        p[0, d] = (snr, n, iw, snr * 2)
    p[0, 4] = (7.999, 1, 0, 1.0)
    p[1, 4] = (9.5, 6, 1, 1.0)
    p[1, 5] = (9.5, 7, 2, 1.0)
    p[1, 0] = (50.0, -1, -1, 0.0)                                               # (not scored, whatever the word holds)
    got = pulse_candidates(p, 8.0, dms, widths)
    assert got == [dict(pair=0, idm=2, dm=1.0, snr=11.0, window=4, iw=2, width=4, ntrial=3),
                   dict(pair=0, idm=5, dm=2.5, snr=8.25, window=0, iw=3, width=8, ntrial=1),
                   dict(pair=0, idm=7, dm=3.5, snr=8.0, window=2, iw=0, width=1, ntrial=1),
                   dict(pair=1, idm=4, dm=2.0, snr=9.5, window=6, iw=1, width=2, ntrial=2)]
    above = pulse_candidates(p, np.nextafter(np.float32(8.0), np.float32(9.0)), dms, widths)
    assert [c['idm'] for c in above if c['pair'] == 0] == [2, 5]
    assert [(c['idm'], c['ntrial']) for c in pulse_candidates(p, 7.0, dms, widths) if c['pair'] == 0] == [(2, 5), (7, 1)]
    # the same plane as raw words, and refusals
    raw = p.reshape(-1).view(np.uint32).reshape(2, 8, 4)
    assert pulse_candidates(raw, 8.0, dms, widths) == got
    assert as_records(p.tobytes(), 2, 8).shape == (2, 8)
    with pytest.raises(ValueError, match="pulse_search"):
        pulse_candidates(p, 8.0, dms[:-1], widths)
    with pytest.raises(ValueError, match="pulse_search"):
        as_records(np.zeros(7, np.uint32))


# ---------------------------------------------------------------- the block on CPU rings
@pytest.mark.parametrize("nprod", [1, 4])
def test_block_spans_within_and_across_sequences(nprod):
    """Source -> BeamPulseSearch -> Sink on in-repo rings, two sequences of 5 spans of 6 windows, nstat = 8.  The baseline and
    the boxcars cross the spans of a sequence and not the sequences; every plane equals the restatement's record of that call;
    the output header adds nwidth, nstat, widths, threshold."""
    npair, ndm, nwin, nspan, nwidth, nstat = 2, 5, 6, 5, 3, 8
    rng = np.random.default_rng(5 + nprod)
    xs = [_noise(rng, nspan * nwin, npair, ndm, nprod) for _ in range(2)]
    hdrs = [dedisp_header(npair, ndm, nprod, seq0=1000 * (s + 1), S=0) for s in range(2)]
    r0, r1 = Ring("dd-output"), Ring("ps-output")
    be = PulseBackend()
    got = []
    ps = BeamPulseSearch(LOG, r0, r1, npair=npair, ndm=ndm, nwin=nwin, nwidth=nwidth, nstat=nstat, threshold=1.5, on_candidates=got.append, backend=be)
    sink = Sink(r1, npair * ndm * 16)
    run_blocks([ps], Source(r0, [(hdrs[s], xs[s], nwin * npair * ndm * nprod * 4) for s in range(2)]), [sink])
    assert len(sink.sequences) == 2
    ncand = 0
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        assert tag == hdrs[s]['seq0'] and hd['seq0'] == hdrs[s]['seq0'] and len(spans) == nspan
        exp = pulse_search(series(xs[s], np.float32), nstat, nwidth, np.float32, [nwin] * nspan)['records']
        for k, o in enumerate(spans):
            assert o.tobytes() == plane_of(exp[k]).tobytes(), (s, k)
            ncand += len(pulse_candidates(plane_of(exp[k]), 1.5, hdrs[s]['dms'], [1, 2, 4]))
        assert (as_records(spans[0], npair, ndm)['n'] == -1).all() and (as_records(spans[2], npair, ndm)['n'] >= 0).all()
    hd = sink.sequences[0][0]
    assert hd['nwidth'] == nwidth and hd['nstat'] == nstat and hd['widths'] == [1, 2, 4] and hd['threshold'] == 1.5
    assert hd['ndm'] == ndm and hd['dedisp_latency'] == 0 and hd['nprod'] == nprod and hd['dms'] == hdrs[0]['dms']
    assert be.calls == [('init', nprod)] + ['run'] * nspan + ['reset'] + ['run'] * nspan
    assert ps.stats['nwindow'] == 2 * nspan * nwin and ps.stats['ncand'] == ncand == sum(len(c) for c in got) and ncand > 0


def test_block_gap_resets_and_restarts_the_output_sequence():
    """Spans 0, 1, 2, 4, 5, 6 of a sequence (3 never read): the context is reset, the output restarts in a sequence of its own at
    span 4's sample, and spans 4-6 are the restatement of a run that begins at span 4."""
    npair, ndm, nwin, nwidth, nstat, seq0, acc_len = 1, 5, 4, 2, 4, 700, 32
    rng = np.random.default_rng(11)
    x = _noise(rng, 7 * nwin, npair, ndm, 1)
    hdr = dedisp_header(npair, ndm, 1, seq0=seq0, acc_len=acc_len)
    seen = [(k, np.ascontiguousarray(x[k * nwin:(k + 1) * nwin])) for k in (0, 1, 2, 4, 5, 6)]
    be = PulseBackend()
    r1 = Ring("ps-output")
    ps = BeamPulseSearch(LOG, _FakeRing([_FakeSeq(hdr, seen, nwin * npair * ndm * 4)]), r1, npair=npair, ndm=ndm, nwin=nwin, nwidth=nwidth, nstat=nstat,
                         backend=be)
    sink = Sink(r1, npair * ndm * 16)
    sink.start()
    ps.main()
    sink.join(20)
    assert be.calls == [('init', 1), 'run', 'run', 'run', 'reset', 'run', 'run', 'run']
    (h0, t0, a), (h1, t1, b) = sink.sequences
    step = nwin * acc_len
    assert (h0['seq0'], t0, h1['seq0'], t1) == (seq0, seq0, seq0 + 4 * step, seq0 + 4 * step) and len(a) == len(b) == 3
    for spans, first in ((a, 0), (b, 4)):
        exp = pulse_search(series(x[first * nwin:(first + 3) * nwin], np.float32), nstat, nwidth, np.float32, [nwin] * 3)['records']
        for k, o in enumerate(spans):
            assert o.tobytes() == plane_of(exp[k]).tobytes()
    assert (as_records(b[0], npair, ndm)['n'] == -1).all() and (as_records(b[1], npair, ndm)['n'] >= 0).all()
    assert ps.stats['ngap'] == 1


def test_block_threshold_command_lands_at_the_next_span():
    """A `threshold` command that arrives after span 1 was enqueued: spans 0 and 1 are judged at 100 (nothing), spans 2 and 3 at
    0.5.  A command that is not a finite number is refused and changes nothing.  The header keeps the threshold of its start."""
    npair, ndm, nwin, nwidth, nstat = 1, 5, 4, 2, 4
    rng = np.random.default_rng(13)
    x = _noise(rng, 4 * nwin, npair, ndm, 1)
    hdr = dedisp_header(npair, ndm, 1, S=0)
    be = PulseBackend()
    r1 = Ring("ps-output")
    box, got = {}, []

    def spans():
        for k in range(4):
            if k == 2:
                box['ps'].process_command_strings(_cmd(0.5))
                assert box['ps'].last_response['val']['status'] == 'normal'
            if k == 3:
                for bad in ("high", float('nan'), [1.0], None):
                    box['ps'].process_command_strings(_cmd(bad, "2"))
                    assert box['ps'].last_response['val']['status'] == 'error'
            yield k, np.ascontiguousarray(x[k * nwin:(k + 1) * nwin])

    seq = _FakeSeq(hdr, spans(), nwin * npair * ndm * 4)
    ps = box['ps'] = BeamPulseSearch(LOG, _FakeRing([seq]), r1, npair=npair, ndm=ndm, nwin=nwin, nwidth=nwidth, nstat=nstat, threshold=100,
                                     on_candidates=got.append, backend=be)
    sink = Sink(r1, npair * ndm * 16)
    sink.start()
    ps.main()
    sink.join(20)
    (hd, _, out), = sink.sequences
    assert hd['threshold'] == 100 and len(out) == 4
    exp = [pulse_candidates(as_records(o, npair, ndm), 0.5, hdr['dms'], [1, 2]) for o in out]
    assert len(pulse_candidates(as_records(out[1], npair, ndm), 0.5, hdr['dms'], [1, 2])) > 0
    strip = [[{f: v for f, v in c.items() if f != 'sample'} for c in cs] for cs in got]
    assert strip == [e for e in exp[2:] if e] and len(strip) == 2
    assert ps.stats['threshold'] == 0.5 and ps.threshold == 0.5
    assert ps.stats['candidates'] == got[-1] and ps.stats['ncand'] == sum(len(c) for c in got)


@pytest.mark.parametrize("w", [1, 4])
def test_block_sample_is_the_planted_sample(w):
    """A box of w windows planted at beamformer sample X of the top channel: it arrives in the dedispersed series S windows
    later, window n_start = (X - seq0) / acc_len + S of the sequence, and the one candidate's `sample` is X, with its pair, trial,
    DM and width."""
    npair, ndm, nwin, nwidth, nstat, seq0, acc_len, S = 2, 5, 6, 3, 16, 4096, 32, 5
    rng = np.random.default_rng(17 + w)
    x = _noise(rng, 9 * nwin, npair, ndm, 1)
    X = seq0 + 31 * acc_len
    n_start = (X - seq0) // acc_len + S                                          # (36: the box lies in block 2 and in one span)
    x[n_start:n_start + w, 1, 3, 0] += 600 / w
    x[n_start:n_start + w, 1, 2, 0] += 400 / w                                   # (the neighbouring trial sees it too, fainter)
    hdr = dedisp_header(npair, ndm, 1, seq0=seq0, S=S, acc_len=acc_len)
    got = []
    ps = BeamPulseSearch(LOG, Ring("dd-output"), Ring("ps-output"), npair=npair, ndm=ndm, nwin=nwin, nwidth=nwidth, nstat=nstat, threshold=8.0,
                         on_candidates=got.extend, backend=PulseBackend())
    sink = Sink(ps.oring, npair * ndm * 16)
    run_blocks([ps], Source(ps.iring, [(hdr, x, nwin * npair * ndm * 4)]), [sink])
    assert len(got) == 1, got
    c, = got
    assert (c['pair'], c['idm'], c['dm'], c['width'], c['iw'], c['ntrial']) == (1, 3, 1.5, w, {1: 0, 4: 2}[w], 2)
    assert c['sample'] == X and c['window'] == (n_start + w - 1) % nwin and c['snr'] > 8


def test_block_leaves_out_what_the_dedispersers_first_windows_spoil():
    """The first S = 5 outputs of the dedisperser are partial sums (here: a ramp up to the level of the rest), so block 0 sits
    too low and block 1 is measured against it: boxcars that reach from block 2 back into block 1 score high under block 1's small
    sigma.  The planes hold those records; the candidates leave out every record whose boxcar begins before window
    (ceil(5 / 8) + 1) * 8 = 16, and a pulse planted at window 28 is the one candidate."""
    npair, ndm, nwin, nwidth, nstat, S = 1, 5, 8, 3, 8, 5
    rng = np.random.default_rng(23)
    x = 1000 + _noise(rng, 4 * nwin, npair, ndm, 1)
    x[:S] *= (np.arange(S)[:, None, None, None] + 1) / (S + 1)
    x[28, 0, 2, 0] += 400
    hdr = dedisp_header(npair, ndm, 1, seq0=64, S=S)
    got = []
    ps = BeamPulseSearch(LOG, Ring("dd-output"), Ring("ps-output"), npair=npair, ndm=ndm, nwin=nwin, nwidth=nwidth, nstat=nstat, threshold=8.0,
                         on_candidates=got.extend, backend=PulseBackend())
    sink = Sink(ps.oring, npair * ndm * 16)
    run_blocks([ps], Source(ps.iring, [(hdr, x, nwin * npair * ndm * 4)]), [sink])
    (_, _, planes), = sink.sequences
    raw = [c for k, p in enumerate(planes) for c in pulse_candidates(as_records(p, npair, ndm), 8.0, hdr['dms'], [1, 2, 4])]
    assert len(raw) == 2 and raw[0]['ntrial'] == 5 and ps.stats['nstartup'] == 10          # (the five records of span 1 and of span 2)
    assert [(c['idm'], c['width'], c['sample']) for c in got] == [(2, 1, 64 + (28 - S) * 32)]


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(npair=0), dict(ndm=-1), dict(nwin=0), dict(nwidth=0), dict(nwidth=9), dict(nstat=1), dict(nstat=(1 << 20) + 1),
                                dict(nwidth=6, nstat=31), dict(threshold=float('nan')), dict(threshold="8"), dict(on_candidates=3)])
def test_constructor_refuses_bad_arguments(kw):
    args = dict(npair=1, ndm=5, nwin=4)
    args.update(kw)
    be = PulseBackend()
    with pytest.raises(ValueError, match="BEAM_PULSE_SEARCH"):
        BeamPulseSearch(LOG, Ring("a"), Ring("b"), backend=be, **args)
    assert be.ps is None


def test_constructor_refuses_a_device_output_ring():
    with pytest.raises(ValueError, match="BEAM_PULSE_SEARCH"):
        BeamPulseSearch(LOG, Ring("a"), _FakeOut(), npair=1, ndm=5, nwin=4, backend=PulseBackend())


class _FakeOut:
    name, space = "device-output", "cuda"


@pytest.mark.parametrize("bad", [dict(ndm=None), dict(ndm=4), dict(nbeam=2), dict(nprod=2), dict(nprod=None), dict(tsamp=None), dict(tsamp=0.0),
                                 dict(dms=[0.0]), dict(dedisp_latency=None), dict(dedisp_latency=-1), dict(acc_len=0)])
def test_block_refuses_what_is_not_dedispersed_beams(bad):
    """An input without ndm (it has not been dedispersed), other sizes, products, no window length or latency: ValueError before
    any run."""
    npair, ndm, nwin = 1, 5, 4
    be = PulseBackend()
    hdr = dedisp_header(npair, ndm, 1)
    for k, v in bad.items():
        if v is None:
            del hdr[k]
        else:
            hdr[k] = v
    x = np.zeros((nwin, npair, ndm, 1), np.float32)
    ps = BeamPulseSearch(LOG, _FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), npair=npair, ndm=ndm, nwin=nwin, nwidth=2, nstat=4, backend=be)
    with pytest.raises(ValueError, match="BEAM_PULSE_SEARCH"):
        ps.main()
    assert 'run' not in be.calls


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengPulseInitialize", "xengPulseRun", "xengPulseReset", "xengPulseGetInfo", "xengPulseGetBaseline", "xengPulseCheckGuards", "xengPulseMark",
         "xengPulseWait", "xengPulseTicketDone", "xengPulseSync", "xengPulseDestroy")


def test_backend_forwards_every_call_the_block_makes():
    """HipBackend has a method for each pulse_* call of the block (and the fake backend above has the same ones)."""
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("pulse_initialize", "pulse_run", "pulse_reset", "pulse_info", "pulse_baseline", "pulse_guards_intact", "pulse_mark", "pulse_wait",
              "pulse_ticket_done", "pulse_sync"):
        assert callable(getattr(HipBackend, m)), m
    for m in ("pulse_initialize", "pulse_run", "pulse_reset", "pulse_mark", "pulse_wait", "pulse_sync"):
        assert callable(getattr(PulseBackend, m)), m


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Reset, Mark and TicketDone are enqueue-only, the calls that wait are not.
    Initialize refuses bad sizes, nprod, nwidth, nstat, a boxcar longer than a block and more than a launch takes before it
    touches a device; Run refuses null and misaligned pointers, GetInfo / GetBaseline / CheckGuards / Mark / TicketDone null
    results, before looking for a context; without one, INVALID_STATE."""
    L = ffi.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in ffi.SYMBOLS, name
    for name in ("xengPulseRun", "xengPulseReset", "xengPulseMark", "xengPulseTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengPulseInitialize", "xengPulseGetBaseline", "xengPulseWait", "xengPulseSync", "xengPulseCheckGuards", "xengPulseGetInfo"):
        assert name not in ffi.ENQUEUE_ONLY, name
    # (gpu, npair, ndm, nwin, nprod, nwidth, nstat)
    for args in ((0, 0, 256, 30, 1, 8, 256), (0, 16, 0, 30, 1, 8, 256), (0, 16, 256, 0, 1, 8, 256), (0, 16, 256, 30, 2, 8, 256),
                 (0, 16, 256, 30, 0, 8, 256), (0, 16, 256, 30, 1, 0, 256), (0, 16, 256, 30, 1, 9, 256), (0, 16, 256, 30, 1, 8, 1),
                 (0, 16, 256, 30, 1, 8, (1 << 20) + 1), (0, 16, 256, 30, 1, 8, 127), (0, 16, 256, 30, 1, 3, 3), (0, 1 << 13, 1 << 12, 30, 1, 8, 256),
                 (0, 16, 256, 65, 1, 8, 256), (0, 16, 256, 129, 1, 1, 256)):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengPulseInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    f = np.zeros(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    n = ctypes.c_longlong()
    for name, args in (("xengPulseRun", (None, 1, 4096)), ("xengPulseRun", (4096, 1, None)), ("xengPulseRun", (4100, 1, 4096)),
                       ("xengPulseRun", (4096, 1, 4104)), ("xengPulseGetInfo", (None, ctypes.byref(n))), ("xengPulseGetInfo", (ctypes.byref(n), None)),
                       ("xengPulseGetBaseline", (None, f, f)), ("xengPulseGetBaseline", (f, None, f)), ("xengPulseGetBaseline", (f, f, None)),
                       ("xengPulseMark", (None,)), ("xengPulseTicketDone", (1, None)), ("xengPulseCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_pulse_gpu.py covers the rest)
    s, t = ctypes.c_int(), ctypes.c_ulonglong()
    for name, args in (("xengPulseRun", (4096, 1, 4096)), ("xengPulseReset", ()), ("xengPulseGetInfo", (ctypes.byref(n), ctypes.byref(n))),
                       ("xengPulseGetBaseline", (f, f, f)), ("xengPulseMark", (ctypes.byref(t),)), ("xengPulseWait", (1,)),
                       ("xengPulseTicketDone", (1, ctypes.byref(s))), ("xengPulseSync", ()), ("xengPulseCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengPulseDestroy")       # (nothing to destroy: success)
