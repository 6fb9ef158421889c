"""BeamCoherentDedisperseLong without a GPU: cdedisp_plan_long's choices and refusals; the block on fake rings with a backend that
serves cdlong_* from the restatement (tests/cdlong_ref.py) -- planned and explicit plans, the header keys, one span per block, a gap,
a `dms` command that uploads every pair, the constructor's refusals -- and the C entry points' bindings and argument checks."""
import ctypes
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi
from caltech_bifrost_dsp_amd.blocks import BeamCoherentDedisperse, BeamCoherentDedisperseLong, cdedisp_plan, cdedisp_plan_long, chirp_table, smear_samples
from caltech_bifrost_dsp_amd.blocks.coherent_dedisp import NFFT_LONG_MAX, NFFT_LONG_MIN
from caltech_bifrost_dsp_amd.ring import Ring
from tests.cdedisp_ref import filter_blocks, gaussian_rows, nblocks_after, select
from tests.cdlong_ref import CdlongBackend
from tests.pipeline_util import LOG, Sink, source_header
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
CHAN_BW = 23925.78125
NCHAN, NBEAM, PAIR0, NPAIR, G, NFFT, M = 2, 6, 1, 2, 4000, 1 << 14, 4560       # a selection offset, gulps unrelated to L
L = NFFT - M
UNIT = NCHAN * 2 * NPAIR * L * 8
DMS = [4.0, 8.0]                                # (at 25 MHz sweeps of 1216 and 2432 samples: within M)
SFREQ = 25e6


def voltage_header(nchan=NCHAN, nbeam=NBEAM, seq0=0, sfreq=SFREQ, **extra):
    """The sequence header Beamform writes for its voltage output."""
    hdr = source_header(nchan, nbeam, 1, seq0=seq0, sfreq=sfreq, chan_bw=CHAN_BW)
    hdr.update(nbeam=nbeam, nstand=nbeam, npol=1, nbit=32, complex=True)
    hdr.update(extra)
    return hdr


def _gulps(v, g):
    return [np.ascontiguousarray(v[..., k * g:(k + 1) * g]) for k in range(v.shape[-1] // g)]


def _table(hdr, dms, nfft=NFFT):
    return chirp_table(hdr['sfreq'] + CHAN_BW * np.arange(hdr['nchan']), CHAN_BW, dms, nfft)


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


def _units(spans, nchan=NCHAN, nb=2 * NPAIR, step=L):
    return np.array([s.view(np.complex64).reshape(nchan, nb, step) for s in spans])


def _block(iring, oring, be, **kw):
    args = dict(nchan=NCHAN, nbeam=NBEAM, ntime_gulp=G, dms=DMS, pair0=PAIR0, npair=NPAIR, nfft=NFFT, overlap=M)
    args.update(kw)
    return BeamCoherentDedisperseLong(LOG, iring, oring, backend=be, **args)


def _run(cd, oring, unit):
    sink = Sink(oring, unit)
    sink.start()
    cd.main()
    sink.join(20)
    return sink.sequences


# ---------------------------------------------------------------- the plan
def test_cdedisp_plan_long_choices_and_refusals():
    """cdedisp_plan's rule over 2^14 .. 2^20: an even M of at least 1.5 sweeps of the lowest channel within half the transform, the
    step a multiple of `multiple_of`, the smallest transform that fits.  23.9 kHz channels: 2^14 at 25 MHz and DM 10 (which
    cdedisp_plan refuses), 2^15 at 20 MHz, 2^16 at 15 MHz, 2^17 at 20 MHz and the Crab's DM."""
    band = lambda f: f + CHAN_BW * np.arange(4)
    assert (NFFT_LONG_MIN, NFFT_LONG_MAX) == (1 << 14, 1 << 20)
    for f, dm, nfft in ((25e6, 10.0, 1 << 14), (20e6, 10.0, 1 << 15), (15e6, 10.0, 1 << 16), (20e6, 56.8, 1 << 17), (20e6, -56.8, 1 << 17)):
        sweep = float(np.max(smear_samples(band(f), CHAN_BW, dm)))
        for mult in (1, 8, 48):
            n, m = cdedisp_plan_long(band(f), CHAN_BW, dm, mult)
            assert n == nfft and m % 2 == 0 and 1.5 * sweep <= m <= n // 2 and (n - m) % mult == 0, (f, dm, mult, n, m)
            assert m < 1.5 * sweep + 2 * mult + 2                               # (of those M the smallest)
        if nfft > 1 << 14:
            assert 1.5 * sweep > nfft // 4                                      # (the transform below it does not fit)
    assert cdedisp_plan_long(band(25e6), CHAN_BW, 10.0) == (1 << 14, 4560)      # sweep 3040 -> 4560, as the issue's table
    assert cdedisp_plan_long(band(50e6), CHAN_BW, 10.0) == (1 << 14, 570)       # (a short sweep still gets the long engine's 2^14)
    with pytest.raises(ValueError, match="cdedisp_plan"):
        cdedisp_plan(band(25e6), CHAN_BW, 10.0)                                 # (the old planner keeps refusing it)
    with pytest.raises(ValueError, match="cdedisp_plan_long"):
        cdedisp_plan_long(band(12e6), CHAN_BW, 500.0)
    with pytest.raises(ValueError, match="cdedisp_plan_long"):
        cdedisp_plan_long(band(25e6), CHAN_BW, 10.0, 0)


# ---------------------------------------------------------------- the block on fake rings
@pytest.mark.parametrize("planned", [False, True])
def test_block_one_span_per_block_header_and_seq0(planned):
    """Two sequences of 12 gulps of 4000 samples through BeamCoherentDedisperseLong with an explicit plan (2^14, 4560) and with the
    plan made at the first sequence (25 MHz, DMs 4 and 10, multiple_of 8: (2^14, 4560) again, 11824 = 8 * 1478): every output span
    is one block of the restatement, as many as nblocks_after says; the header is the input's with nbeam = nstand = 4, pair0, the
    three cdedisp_ keys and seq0 = the input's + M/2, which is the time tag too; every pair's table is uploaded by a call of its
    own, and the context is made through cdlong_initialize."""
    dms = [4.0, 10.0] if planned else DMS
    n = 12 * G
    rng = np.random.default_rng(11)
    xs = [gaussian_rows(rng, NCHAN, NBEAM, n) for _ in range(2)]
    hdrs = [voltage_header(seq0=1000 * (s + 1)) for s in range(2)]
    be = CdlongBackend()
    seen = []
    real_init = be.cdedisp_initialize
    be.cdlong_initialize = lambda *a: (seen.append('cdlong_initialize'), real_init(*a))[1]
    r1 = Ring("cd-output")
    kw = dict(dms=dms, nfft=None, overlap=None, multiple_of=8) if planned else {}
    cd = _block(_FakeRing([_FakeSeq(hdrs[s], list(enumerate(_gulps(xs[s], G))), NCHAN * NBEAM * G * 8) for s in range(2)]), r1, be, **kw)
    assert (be.cd is None) == planned
    if planned:
        assert cdedisp_plan_long(SFREQ + CHAN_BW * np.arange(NCHAN), CHAN_BW, 10.0, 8) == (NFFT, M)
    seqs = _run(cd, r1, UNIT)
    nblk = nblocks_after(n, NFFT, M)
    assert len(seqs) == 2 and nblk == 3 and seen == ['cdlong_initialize'] and (be.cd['nfft'], be.cd['overlap']) == (NFFT, M)
    for s, (hd, tag, spans) in enumerate(seqs):
        assert tag == hd['seq0'] == hdrs[s]['seq0'] + M // 2 and len(spans) == nblk
        exp = filter_blocks(select(xs[s], PAIR0, NPAIR), _table(hdrs[s], dms), NFFT, M, np.complex64)
        assert _units(spans).tobytes() == exp.tobytes()
        assert (hd['nbeam'], hd['nstand'], hd['pair0'], hd['cdedisp_dm'], hd['cdedisp_nfft'], hd['cdedisp_overlap']) == (4, 4, PAIR0, dms, NFFT, M)
        assert hd['nchan'] == NCHAN and hd['sfreq'] == hdrs[s]['sfreq'] and not {'acc_len', 'ntime_sum', 'nupchan'} & set(hd)
    per = ['run%d' % (nblocks_after((k + 1) * G, NFFT, M) - nblocks_after(k * G, NFFT, M)) for k in range(n // G)]
    assert be.calls == ['init', 'reset', 'chirp0', 'chirp1'] + per + ['reset', 'chirp0', 'chirp1'] + per
    assert sorted(set(per)) == ['run0', 'run1'] and cd.stats['nblock'] == 2 * nblk and cd.stats['ndropped'] == 0


def test_block_gap_restarts_the_stream_in_a_sequence_of_its_own():
    """Gulps 0..5 and 7..15 of a sequence (6 never read): block 0 completes by gulp 5 (16384 of 24000 samples), the second is in
    progress and the gap drops it (ndropped = 1); the context is reset and the output restarts in a sequence of its own whose seq0
    is gulp 7's sample + M/2, with the blocks of a stream that begins there."""
    rng = np.random.default_rng(7)
    x = gaussian_rows(rng, NCHAN, NBEAM, 16 * G)
    hdr = voltage_header(seq0=300)
    gulps = _gulps(x, G)
    seen = [(k, gulps[k]) for k in list(range(6)) + list(range(7, 16))]
    be = CdlongBackend()
    r1 = Ring("cd-output")
    cd = _block(_FakeRing([_FakeSeq(hdr, seen, NCHAN * NBEAM * G * 8)]), r1, be)
    (h0, t0, a), (h1, t1, b) = _run(cd, r1, UNIT)
    assert (h0['seq0'], t0, h1['seq0'], t1) == (300 + M // 2, 300 + M // 2, 300 + 7 * G + M // 2, 300 + 7 * G + M // 2)
    rows = select(x, PAIR0, NPAIR)
    assert len(a) == nblocks_after(6 * G, NFFT, M) == 1 and len(b) == nblocks_after(9 * G, NFFT, M) == 2
    assert _units(a).tobytes() == filter_blocks(rows[..., :6 * G], _table(hdr, DMS), NFFT, M, np.complex64).tobytes()
    assert _units(b).tobytes() == filter_blocks(rows[..., 7 * G:], _table(hdr, DMS), NFFT, M, np.complex64).tobytes()
    assert be.calls.count('reset') == 2 and be.calls.index('reset', 2) == 4 + 6 and cd.stats['ndropped'] == 1 and cd.stats['nblock'] == 3


def test_block_dms_command_restarts_the_sequence_and_uploads_every_pair():
    """A `dms` command before gulp 6: block 0 (complete by then) carries the first table, every later block of the SAME stream the
    new one, and the output restarts in a sequence of its own at block 1's first sample, whose header says the new DMs.  Every
    pair's table is uploaded again, the unchanged pair's too."""
    rng = np.random.default_rng(9)
    x = gaussian_rows(rng, NCHAN, NBEAM, 12 * G)
    hdr = voltage_header(seq0=40)
    new = [DMS[0], 2.0]
    box = {}

    def spans():
        for k, a in enumerate(_gulps(x, G)):
            if k == 6:
                box['cd'].process_command_strings(_cmd(dms=new))
                assert box['cd'].last_response['val']['status'] == 'normal'
            if k == 8:
                box['cd'].process_command_strings(_cmd("2", dms=[0.1]))
                assert box['cd'].last_response['val']['status'] == 'error'
            yield k, a

    be = CdlongBackend()
    r1 = Ring("cd-output")
    cd = box['cd'] = _block(_FakeRing([_FakeSeq(hdr, spans(), NCHAN * NBEAM * G * 8)]), r1, be)
    (h0, t0, a), (h1, t1, b) = _run(cd, r1, UNIT)
    rows = select(x, PAIR0, NPAIR)
    assert (h0['cdedisp_dm'], h1['cdedisp_dm']) == (DMS, new) and t0 == h0['seq0'] == 40 + M // 2 and t1 == h1['seq0'] == 40 + L + M // 2
    assert len(a) == 1 and len(b) == nblocks_after(12 * G, NFFT, M) - 1 == 2
    assert _units(a).tobytes() == filter_blocks(rows, _table(hdr, DMS), NFFT, M, np.complex64, 0, 1).tobytes()
    assert _units(b).tobytes() == filter_blocks(rows, _table(hdr, new), NFFT, M, np.complex64, 1, 2).tobytes()
    assert be.calls[:4] == ['init', 'reset', 'chirp0', 'chirp1'] and be.calls[4 + 6:4 + 8] == ['chirp0', 'chirp1']
    assert be.calls.count('chirp0') == be.calls.count('chirp1') == 2 and be.calls.count('reset') == 1
    assert cd.dms == new and cd.stats['dms'] == new and cd.stats['nblock'] == 3


@pytest.mark.parametrize("kw", [dict(nfft=1 << 13, overlap=2048), dict(nfft=1 << 21), dict(nfft=3 << 13), dict(overlap=4561), dict(overlap=(1 << 13) + 2),
                                dict(overlap=-2), dict(overlap=None), dict(multiple_of=7), dict(multiple_of=0), dict(nchan=0), dict(pair0=2, npair=2),
                                dict(dms=[0.1])])
def test_constructor_refuses_bad_arguments(kw):
    """nfft 2^13 (the other block's), 2^21 and 3 * 2^13; an odd overlap and one above nfft/2; a step (11824 = 2^4 * 739) that is no
    multiple of multiple_of: ValueError that names this block, and no context made."""
    be = CdlongBackend()
    with pytest.raises(ValueError, match="BEAM_COHERENT_DEDISPERSE_LONG"):
        _block(Ring("a"), Ring("b"), be, **kw)
    assert be.cd is None


def test_the_short_block_keeps_its_limits_and_its_name():
    """The hooks the long block hangs on leave BeamCoherentDedisperse what it was: 2^14 refused under its own name, its backend
    methods cdedisp_*."""
    be = CdlongBackend()
    with pytest.raises(ValueError, match=r"BEAM_COHERENT_DEDISPERSE: nfft 16384 is not a power of two from 2\^8 to 2\^13"):
        BeamCoherentDedisperse(LOG, Ring("a"), Ring("b"), NCHAN, NBEAM, G, DMS, pair0=PAIR0, npair=NPAIR, nfft=NFFT, overlap=M, backend=be)
    BeamCoherentDedisperse(LOG, Ring("a"), Ring("b"), NCHAN, NBEAM, G, DMS, pair0=PAIR0, npair=NPAIR, nfft=256, overlap=64, backend=be)
    assert be.calls == ['init'] and issubclass(BeamCoherentDedisperseLong, BeamCoherentDedisperse)


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("Initialize", "SetChirp", "Run", "Reset", "GetInfo", "CheckGuards", "Mark", "Wait", "TicketDone", "Sync", "Destroy")


def test_backend_forwards_every_call_the_block_makes():
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("initialize", "set_chirp", "run", "reset", "info", "guards_intact", "mark", "wait", "sync"):
        assert callable(getattr(HipBackend, "cdlong_" + m)), m
    for m in ("initialize", "set_chirp", "run", "reset", "mark", "wait", "sync"):
        assert callable(getattr(CdlongBackend, "cdlong_" + m)), m


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each xengCdlong* symbol is exported and bound, and enqueue-only exactly where its xengCdedisp* twin is.  Initialize refuses
    every size outside the contract before it touches a device -- 2^13 and 2^21 among them, and nchan * 2 npair > 65535; Run
    refuses null and misaligned pointers, the getters null results, SetChirp a null table and a negative pair, before looking for
    a context; without one, INVALID_STATE."""
    lib = ffi.lib()
    for n in NAMES:
        name, twin = "xengCdlong" + n, "xengCdedisp" + n
        assert hasattr(lib, name) and name in ffi.SYMBOLS, name
        assert (name in ffi.ENQUEUE_ONLY) == (twin in ffi.ENQUEUE_ONLY), name
    assert [n for n in NAMES if "xengCdlong" + n in ffi.ENQUEUE_ONLY] == ["Run", "Reset", "Mark", "TicketDone"]
    # (gpu, nchan, nbeam, ntime, pair0, npair, nfft, overlap)
    good = (0, 96, 32, 480, 0, 16, 1 << 17, 40000)
    for i, v in ((1, 0), (2, 0), (3, 0), (4, -1), (4, 1), (5, 0), (5, 17), (6, 1 << 13), (6, 1 << 21), (6, 3 << 15), (6, 100000), (7, -2), (7, 39999),
                 (7, (1 << 16) + 2), (1, 2048), (6, 1 << 20), (3, 1 << 30)):     # (96 x 16 pairs at 2^20: a state of 64 GB)
        args = list(good)
        args[i] = v
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCdlongInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    n, s = ctypes.c_longlong(), ctypes.c_int()
    f = np.zeros(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for name, args in (("xengCdlongRun", (None, 4096, ctypes.byref(s))), ("xengCdlongRun", (4096, 4096, None)),
                       ("xengCdlongRun", (4104, 4096, ctypes.byref(s))), ("xengCdlongRun", (4096, 4104, ctypes.byref(s))),
                       ("xengCdlongGetInfo", (None, ctypes.byref(s), ctypes.byref(n), ctypes.byref(n))),
                       ("xengCdlongGetInfo", (ctypes.byref(s), None, ctypes.byref(n), ctypes.byref(n))),
                       ("xengCdlongGetInfo", (ctypes.byref(s), ctypes.byref(s), None, ctypes.byref(n))),
                       ("xengCdlongGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(n), None)),
                       ("xengCdlongSetChirp", (0, None)), ("xengCdlongSetChirp", (-1, f)), ("xengCdlongMark", (None,)),
                       ("xengCdlongTicketDone", (1, None)), ("xengCdlongCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_cdlong_gpu.py covers the rest)
    t = ctypes.c_ulonglong()
    for name, args in (("xengCdlongRun", (4096, 4096, ctypes.byref(s))), ("xengCdlongRun", (4096, None, ctypes.byref(s))), ("xengCdlongReset", ()),
                       ("xengCdlongSetChirp", (0, f)), ("xengCdlongGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(n), ctypes.byref(n))),
                       ("xengCdlongMark", (ctypes.byref(t),)), ("xengCdlongWait", (1,)), ("xengCdlongTicketDone", (1, ctypes.byref(s))),
                       ("xengCdlongSync", ()), ("xengCdlongCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengCdlongDestroy")       # (nothing to destroy: success)
