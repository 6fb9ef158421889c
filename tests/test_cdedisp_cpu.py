"""BeamCoherentDedisperse without a GPU: chirp_table's group delay, modulus and DM 0; cdedisp_plan's choices and refusals; the
restatement (tests/cdedisp_ref.py) bringing an impulse dispersed in float64 back into one sample; fold_rotations_coherent against
fold_rotations, and BeamFold.rotations with and without the header key; the block on CPU rings (both implementations) with a backend
that serves cdedisp_* from the restatement -- header keys, the seq0 shift, gulps that complete no, one and several blocks, a gap, a
`dms` command, the plan made at the sequence, a downstream UpchanSumBeams that accepts the header, refusals -- and the C entry
points' argument checks."""
import ctypes
import json

import numpy as np
import pytest

import caltech_bifrost_dsp_amd  # noqa: F401
from caltech_bifrost_dsp_amd import ffi, ring
from caltech_bifrost_dsp_amd.blocks import (BeamCoherentDedisperse, BeamFold, UpchanSumBeams, cdedisp_plan, chirp_table, fold_rotations,
                                            fold_rotations_coherent, smear_samples)
from caltech_bifrost_dsp_amd.blocks.dedisp import KDM
from caltech_bifrost_dsp_amd.ndarray import copy_array
from caltech_bifrost_dsp_amd.ring import Ring
from tests.cdedisp_ref import CdedispBackend, disperse, filter_blocks, gaussian_rows, nblocks_after, select
from tests.pipeline_util import LOG, Sink, Source, run_blocks, source_header
from tests.test_dedisp_cpu import power_header
from tests.test_fold_cpu import FoldBackend
from tests.test_upchan_beams_cpu import SumBeamsBackend
from tests.test_upchan_pfb_cpu import _FakeRing, _FakeSeq

INVALID_ARGUMENT, INVALID_STATE = 1, 2          # include/xeng.h XENG_STATUS_*
CHAN_BW = 23925.78125
NCHAN, NBEAM, PAIR0, NPAIR, G, NFFT, M = 3, 6, 1, 2, 100, 256, 64      # the GPU test's common shape
L = NFFT - M
UNIT = NCHAN * 2 * NPAIR * L * 8
DMS = [0.05, 0.1]                               # (at 50 MHz a sweep of 2 and 4 samples: the table is not trivial and fits M)


@pytest.fixture(params=["native", "python"])
def ring_impl(request):
    was = ring.IMPLEMENTATION
    ring.IMPLEMENTATION = request.param
    try:
        yield request.param
    finally:
        ring.IMPLEMENTATION = was


def voltage_header(nchan=NCHAN, nbeam=NBEAM, seq0=0, sfreq=50e6, **extra):
    """The sequence header Beamform writes for its voltage output."""
    hdr = source_header(nchan, nbeam, 1, seq0=seq0, sfreq=sfreq, chan_bw=CHAN_BW)
    hdr.update(nbeam=nbeam, nstand=nbeam, npol=1, nbit=32, complex=True)
    hdr.update(extra)
    return hdr


def _gulps(v, g):
    return [np.ascontiguousarray(v[..., k * g:(k + 1) * g]) for k in range(v.shape[-1] // g)]


def _ring_bytes(v, g):
    return np.concatenate([a.reshape(-1) for a in _gulps(v, g)])


def _table(hdr, dms, nfft=NFFT):
    return chirp_table(hdr['sfreq'] + CHAN_BW * np.arange(hdr['nchan']), CHAN_BW, dms, nfft)


def _cmd(seq_id="1", **kwargs):
    return json.dumps({'cmd': 'update', 'id': seq_id, 'val': {'kwargs': kwargs}})


def _units(spans):
    return np.array([s.view(np.complex64).reshape(NCHAN, 2 * NPAIR, L) for s in spans])


# ---------------------------------------------------------------- the table
@pytest.mark.parametrize("f_c,dm,nfft", [(50e6, 10.0, 2048), (40e6, 10.0, 4096), (30e6, 10.0, 8192), (70e6, -3.0, 256)])
def test_chirp_table_group_delay_modulus_and_dm_zero(f_c, dm, nfft):
    """-(1 / 2 pi) dphi/dnu of the table, by differencing the unwrapped phase between neighbouring bins in ascending frequency,
    against -KDM DM ((f_c + nu)^-2 - f_c^-2) at the midpoints, in samples: within one sample at the band's edges (the difference
    quotient over one bin is exact to second order; the rest is the complex64 rounding of the table, 6e-8 * nfft / 2 pi samples),
    negative below the centre and positive above for a positive DM: what arrived late is moved forward.  |T| nfft = 1; DM 0 gives
    1 / nfft exactly."""
    T = chirp_table([f_c, f_c + CHAN_BW], CHAN_BW, [dm, 0.0], nfft)
    assert T.dtype == np.complex64 and T.shape == (2, 2, nfft)
    assert np.max(np.abs(np.abs(T.astype(np.complex128)) * nfft - 1)) < 2e-7
    assert (T[1] == np.complex64(1.0 / nfft)).all()
    nu = np.fft.fftshift(np.fft.fftfreq(nfft)) * CHAN_BW                        # Hz, ascending
    phi = np.unwrap(np.angle(np.fft.fftshift(T[0, 0].astype(np.complex128))))
    gd = -np.diff(phi) / (2 * np.pi * np.diff(nu)) * CHAN_BW                    # samples
    mid = (0.5 * (nu[1:] + nu[:-1]) + f_c) * 1e-6
    exp = -KDM * dm * (mid ** -2 - (f_c * 1e-6) ** -2) * CHAN_BW
    assert np.max(np.abs(gd - exp)) < 1.0
    assert abs(gd[0] - exp[0]) < 1.0 and abs(gd[-1] - exp[-1]) < 1.0
    assert np.sign(gd[0]) == -np.sign(dm) and np.sign(gd[-1]) == np.sign(dm)
    sweep = smear_samples([f_c], CHAN_BW, dm)[0]
    assert abs((gd[-1] - gd[0]) * np.sign(dm) - sweep) < 0.01 * sweep + 2       # (edge to edge but for half a bin either side)
    for bad in (dict(freqs_hz=[0.0]), dict(dms=[float('nan')]), dict(nfft=300), dict(chan_bw_hz=0.0), dict(dms=[])):
        kw = dict(freqs_hz=[f_c], chan_bw_hz=CHAN_BW, dms=[dm], nfft=nfft)
        kw.update(bad)
        with pytest.raises(ValueError, match="chirp_table"):
            chirp_table(**kw)


def test_smear_samples_are_the_issues_figures():
    """KDM DM (f_lo^-2 - f_hi^-2) in samples of 41.8 us at DM 10: 380 at 50 MHz, 742 at 40 MHz, 1759 at 30 MHz."""
    got = smear_samples([50e6, 40e6, 30e6], CHAN_BW, 10.0)
    assert np.rint(got).tolist() == [380, 742, 1759]
    assert np.array_equal(smear_samples([50e6], CHAN_BW, -10.0), got[:1]) and smear_samples([50e6], CHAN_BW, 0.0)[0] == 0


def test_cdedisp_plan_choices_and_refusals():
    """The smallest power of two that takes an even overlap of at least 1.5 sweeps of the lowest channel within its half, the
    smallest such overlap whose step is a multiple of `multiple_of`; no plan beyond 2^13 points."""
    band = lambda f: f + CHAN_BW * np.arange(4)
    assert cdedisp_plan(band(50e6), CHAN_BW, 10.0) == (2048, 570)               # sweep 380 -> 570
    assert cdedisp_plan(band(50e6), CHAN_BW, 10.0, 8) == (2048, 576)
    assert cdedisp_plan(band(50e6), CHAN_BW, 10.0, 64) == (2048, 576)
    assert cdedisp_plan(band(40e6), CHAN_BW, 10.0) == (4096, 1114)              # sweep 742 -> 1113
    assert cdedisp_plan(band(40e6), CHAN_BW, -10.0, 32) == (4096, 1120)
    assert cdedisp_plan(band(30e6), CHAN_BW, 10.0) == (8192, 2640)              # sweep 1759 -> 2638.8
    assert cdedisp_plan(band(50e6), CHAN_BW, 0.0) == (256, 0)
    assert cdedisp_plan(band(50e6), CHAN_BW, 0.0, 48) == (256, 16)              # (256 - 16 = 5 * 48)
    assert cdedisp_plan(band(50e6), CHAN_BW, 3.4, 1) == (512, 194)              # sweep 129.2: 1.5 x is 193.8, above 256 / 2
    for nfft, m in (cdedisp_plan(band(f), CHAN_BW, 10.0, 8) for f in (60e6, 45e6, 35e6)):
        assert m % 2 == 0 and m <= nfft // 2 and (nfft - m) % 8 == 0
    with pytest.raises(ValueError, match="cdedisp_plan"):
        cdedisp_plan(band(25e6), CHAN_BW, 10.0)                                 # sweep 3040: 4560 > 4096
    with pytest.raises(ValueError, match="cdedisp_plan"):
        cdedisp_plan(band(50e6), CHAN_BW, 10.0, 8191)                           # (the only step would be 8191: an odd overlap)
    with pytest.raises(ValueError, match="cdedisp_plan"):
        cdedisp_plan(band(50e6), CHAN_BW, 10.0, 0)


def _impulse_energy(f_c, dm, nfft, m, t0, nblk=3):
    """An impulse at input sample t0 dispersed in float64, filtered by the float64 restatement with chirp_table's table: (index of
    the largest output sample, its share of the output's energy)."""
    step = nfft - m
    x = np.zeros(nfft + (nblk - 1) * step, np.complex128)
    x[t0] = 1.0
    d = disperse(x, f_c, CHAN_BW, dm, KDM)
    rows = np.stack([d, 0 * d])[None]                                           # (one channel, one pair)
    y = filter_blocks(rows, chirp_table([f_c], CHAN_BW, [dm], nfft), nfft, m)[:, 0, 0].reshape(-1)
    p = np.abs(y) ** 2
    return int(np.argmax(p)), float(p.max() / p.sum())


def test_reference_recovers_a_dispersed_impulse_at_the_planned_overlap():
    """40 MHz, DM 10 (sweep 742), the plan's NFFT 4096 and M 1114 (1.5 sweeps) and the GPU test's M 1216: an impulse dispersed in
    float64 comes back in the sample it was sent in (output sample i is input sample i + M/2), mid-block and two samples from
    either edge of block 1's output.  Measured share of the output's energy in that one sample: 0.99998 mid-block at either M,
    0.99995 at the edges with M 1114 and 0.99996 with M 1216 (the rest is the channel's band edge, where the chirp's spectrum is cut
    off); with M = one sweep (742) it drops to 0.9984 at an edge."""
    f_c, dm = 40e6, 10.0
    nfft, m_plan = cdedisp_plan([f_c], CHAN_BW, dm)
    assert (nfft, m_plan) == (4096, 1114)
    for m in (m_plan, 1216):
        step = nfft - m
        for where, i_out in (("mid", step + step // 2), ("head", step + 2), ("tail", 2 * step - 3)):
            t0 = i_out + m // 2
            at, share = _impulse_energy(f_c, dm, nfft, m, t0)
            print("M %d %s: output sample %d, energy share %.5f" % (m, where, at, share))
            assert at == i_out and share > 0.9998, (m, where, at, share)
    at, share = _impulse_energy(f_c, dm, nfft, 742, 4096 - 742 + 2 + 371)
    print("M 742 head: energy share %.5f" % share)
    assert share < 0.9995                                                       # (the margin is not idle)


# ---------------------------------------------------------------- the fold's rotations
def test_fold_rotations_coherent_against_fold_rotations():
    """dm_coh = dm: fold_rotations at the coarse centres, word for word (the fine channels are aligned already).  dm_coh = 0:
    fold_rotations at the fine centres to within one bin mod nbin (one more sum is rounded).  In between, the formula."""
    hdr = power_header(3, 2, 8, 4)
    nfine, nup, nbin, dm, f_spin = 24, 8, 64, 30.0, 1.4
    freqs = hdr['fine_sfreq'] + hdr['fine_bw_hz'] * np.arange(nfine)
    coarse = hdr['fine_sfreq'] + hdr['fine_bw_hz'] * nup * (np.arange(nfine) // nup + 0.5)
    assert np.allclose(coarse[::nup], hdr['sfreq'] + hdr['bw_hz'] / hdr['nchan'] * np.arange(3))
    got = fold_rotations_coherent(freqs, coarse, dm, dm, f_spin, nbin)
    assert got.dtype == np.int32 and got.tolist() == fold_rotations(coarse, dm, f_spin, nbin, f_ref_hz=freqs.max()).tolist()
    assert len(set(got[:nup].tolist())) == 1 and len(set(got.tolist())) == 3
    d = (fold_rotations_coherent(freqs, coarse, dm, 0.0, f_spin, nbin) - fold_rotations(freqs, dm, f_spin, nbin)) % nbin
    assert set(d.tolist()) <= {0, 1, nbin - 1}
    f, fc, fr = freqs * 1e-6, coarse * 1e-6, freqs.max() * 1e-6
    exp = np.rint(KDM * (dm * (fc ** -2 - fr ** -2) + (dm - 12.5) * (f ** -2 - fc ** -2)) * f_spin * nbin) % nbin
    d = (fold_rotations_coherent(freqs, coarse, dm, 12.5, f_spin, nbin) - exp) % nbin
    assert set(d.tolist()) <= {0, 1, nbin - 1}
    for bad in (dict(dm_coh=float('inf')), dict(coarse_freqs_hz=coarse[:-1]), dict(nbin=0), dict(f_spin=-1.0), dict(f_ref_hz=0.0)):
        kw = dict(freqs_hz=freqs, coarse_freqs_hz=coarse, dm=dm, dm_coh=dm, f_spin=f_spin, nbin=nbin)
        kw.update(bad)
        with pytest.raises(ValueError, match="fold_rotations_coherent"):
            fold_rotations_coherent(**kw)


def test_beam_fold_rotations_with_and_without_the_header_key():
    """Without `cdedisp_dm` BeamFold.rotations is what it was; with it, fold_rotations_coherent at the pair's coherent DM, the
    header's pair0 (what the upchanneliser selected of the dedisperser's pairs) counting into the list."""
    nchan, nup, nbin = 3, 8, 64
    hdr = power_header(nchan, 2, nup, 4)
    psr = [dict(f0=1.4, dm=30.0), None]
    fo = BeamFold(LOG, Ring("a"), Ring("b"), npair=2, nchan=nchan, nupchan=nup, nwin=4, nbin=nbin, pulsars=psr, nsub=1, backend=FoldBackend())
    freqs = hdr['fine_sfreq'] + hdr['fine_bw_hz'] * np.arange(nchan * nup)
    coarse = hdr['sfreq'] + hdr['bw_hz'] / nchan * (np.arange(nchan * nup) // nup)
    plain = fo.rotations(hdr)
    assert plain[0].tolist() == fold_rotations(freqs, 30.0, 1.4, nbin).tolist() and (plain[1] == 0).all()
    with_key = fo.rotations(dict(hdr, cdedisp_dm=[29.0, 0.0]))
    assert with_key[0].tolist() == fold_rotations_coherent(freqs, coarse, 30.0, 29.0, 1.4, nbin).tolist() and (with_key[1] == 0).all()
    assert with_key[0].tolist() != plain[0].tolist()
    shifted = fo.rotations(dict(hdr, cdedisp_dm=[5.0, 30.0, 0.0], pair0=1))
    assert shifted[0].tolist() == fold_rotations_coherent(freqs, coarse, 30.0, 30.0, 1.4, nbin).tolist()
    with pytest.raises(ValueError, match="cdedisp_dm"):
        fo.rotations(dict(hdr, cdedisp_dm=[5.0]))


# ---------------------------------------------------------------- the block on CPU rings
def _block(iring, oring, be, **kw):
    args = dict(nchan=NCHAN, nbeam=NBEAM, ntime_gulp=G, dms=DMS, pair0=PAIR0, npair=NPAIR, nfft=NFFT, overlap=M)
    args.update(kw)
    return BeamCoherentDedisperse(LOG, iring, oring, backend=be, **args)


class _CopyBackend(CdedispBackend):
    """... with the copy stream of the HIP backend (copy_async / copy_done / copy_wait), here a copy on the spot: the block then
    sends a call that completes several blocks through a device buffer and one copy per span."""

    def copy_async(self, dst, src):
        assert dst.nbytes == src.nbytes == UNIT
        copy_array(dst, src)
        self.calls.append('copy')
        return len(self.calls)

    def copy_done(self, stamp):
        return True

    def copy_wait(self, stamp):
        pass


@pytest.mark.parametrize("g,backend", [(G, CdedispBackend), (500, CdedispBackend), (500, _CopyBackend)])
def test_block_one_span_per_block_header_and_seq0(ring_impl, g, backend):
    """Source -> BeamCoherentDedisperse -> Sink, two sequences.  Gulps of 100 samples complete no block or one (L = 192), gulps of
    500 two or three: every output span is one block of the restatement; the header is the input's with nbeam = nstand = 4, pair0,
    the three cdedisp_ keys and seq0 = the input's + M/2, which is the time tag too; a downstream UpchanSumBeams(nbeam=4,
    ntime_gulp=L) accepts it, and refuses the same header once it says nupchan."""
    n = 12 * G if g == G else 5 * 500
    rng = np.random.default_rng(g)
    xs = [gaussian_rows(rng, NCHAN, NBEAM, n) for _ in range(2)]
    hdrs = [voltage_header(seq0=1000 * (s + 1)) for s in range(2)]
    r0, r1 = Ring("beam-output"), Ring("cd-output")
    be = backend()
    cd = _block(r0, r1, be, ntime_gulp=g)
    sink = Sink(r1, UNIT)
    run_blocks([cd], Source(r0, [(hdrs[s], _ring_bytes(xs[s], g), NCHAN * NBEAM * g * 8) for s in range(2)]), [sink])
    ncopy = be.calls.count('copy')
    be.calls = [c for c in be.calls if c != 'copy']
    nblk = nblocks_after(n, NFFT, M)
    assert len(sink.sequences) == 2 and nblk == (5 if g == G else 12)
    for s, (hd, tag, spans) in enumerate(sink.sequences):
        assert tag == hd['seq0'] == hdrs[s]['seq0'] + M // 2 and len(spans) == nblk
        exp = filter_blocks(select(xs[s], PAIR0, NPAIR), _table(hdrs[s], DMS), NFFT, M, np.complex64)
        assert _units(spans).tobytes() == exp.tobytes()
        assert (hd['nbeam'], hd['nstand'], hd['pair0'], hd['cdedisp_dm'], hd['cdedisp_nfft'], hd['cdedisp_overlap']) == (4, 4, PAIR0, DMS, NFFT, M)
        assert hd['nchan'] == NCHAN and hd['sfreq'] == hdrs[s]['sfreq'] and not {'acc_len', 'ntime_sum', 'nupchan'} & set(hd)
    per = ['run%d' % (nblocks_after((k + 1) * g, NFFT, M) - nblocks_after(k * g, NFFT, M)) for k in range(n // g)]
    assert be.calls == ['init', 'reset', 'chirp'] + per + ['reset', 'chirp'] + per
    assert max(int(c[3:]) for c in per) == (1 if g == G else 3) and 'run0' in per or g != G
    assert cd.stats['nblock'] == 2 * nblk and cd.stats['ndropped'] == 0
    assert ncopy == (2 * sum(int(c[3:]) for c in per if int(c[3:]) > 1) if backend is _CopyBackend else 0)
    up = UpchanSumBeams(LOG, Ring("x"), Ring("y"), NCHAN, 2 * NPAIR, L, nupchan=8, backend=SumBeamsBackend())
    up._check_header(sink.sequences[0][0])
    with pytest.raises(ValueError, match="nupchan"):
        up._check_header(dict(sink.sequences[0][0], nupchan=8))


def test_block_gap_restarts_the_stream_in_a_sequence_of_its_own(ring_impl):
    """Gulps 0..5 and 7..15 of a sequence (6 never read): blocks 0 and 1 complete by gulp 5 (448 of 600 samples), the third is in
    progress and the gap drops it (ndropped = 1); the context is reset and the output restarts in a sequence of its own whose seq0
    is gulp 7's sample + M/2, with the blocks of a stream that begins there."""
    rng = np.random.default_rng(7)
    x = gaussian_rows(rng, NCHAN, NBEAM, 16 * G)
    hdr = voltage_header(seq0=300)
    gulps = _gulps(x, G)
    seen = [(k, gulps[k]) for k in list(range(6)) + list(range(7, 16))]
    be = CdedispBackend()
    r1 = Ring("cd-output")
    cd = _block(_FakeRing([_FakeSeq(hdr, seen, NCHAN * NBEAM * G * 8)]), r1, be)
    sink = Sink(r1, UNIT)
    sink.start()
    cd.main()
    sink.join(20)
    (h0, t0, a), (h1, t1, b) = sink.sequences
    assert (h0['seq0'], t0, h1['seq0'], t1) == (300 + M // 2, 300 + M // 2, 300 + 7 * G + M // 2, 300 + 7 * G + M // 2)
    rows = select(x, PAIR0, NPAIR)
    assert len(a) == 2 and _units(a).tobytes() == filter_blocks(rows[..., :6 * G], _table(hdr, DMS), NFFT, M, np.complex64).tobytes()
    assert len(b) == 4 and _units(b).tobytes() == filter_blocks(rows[..., 7 * G:], _table(hdr, DMS), NFFT, M, np.complex64).tobytes()
    assert be.calls.count('reset') == 2 and be.calls.index('reset', 2) == 3 + 6 and cd.stats['ndropped'] == 1 and cd.stats['nblock'] == 6


def test_block_dms_command_holds_from_the_next_block(ring_impl):
    """A `dms` command before gulp 5: blocks 0 and 1 (complete by then) carry the first table, every later block of the SAME stream
    the new one, and the output restarts in a sequence of its own at block 2's first sample, whose header says the new DMs.  What
    is not npair finite numbers is refused and changes nothing."""
    rng = np.random.default_rng(9)
    x = gaussian_rows(rng, NCHAN, NBEAM, 12 * G)
    hdr = voltage_header(seq0=40)
    new = [0.2, 0.0]
    box = {}

    def spans():
        for k, a in enumerate(_gulps(x, G)):
            if k == 5:
                box['cd'].process_command_strings(_cmd(dms=new))
                assert box['cd'].last_response['val']['status'] == 'normal'
            if k == 8:
                for n, bad in enumerate(({'dms': [0.1]}, {'dms': [0.1, float('nan')]}, {'dms': "none"}, {'dms': [0.1, "2"]})):
                    box['cd'].process_command_strings(_cmd(str(2 + n), **bad))
                    assert box['cd'].last_response['val']['status'] == 'error', bad
            yield k, a

    be = CdedispBackend()
    r1 = Ring("cd-output")
    cd = box['cd'] = _block(_FakeRing([_FakeSeq(hdr, spans(), NCHAN * NBEAM * G * 8)]), r1, be)
    sink = Sink(r1, UNIT)
    sink.start()
    cd.main()
    sink.join(20)
    (h0, t0, a), (h1, t1, b) = sink.sequences
    rows = select(x, PAIR0, NPAIR)
    assert (h0['cdedisp_dm'], h1['cdedisp_dm']) == (DMS, new) and t0 == h0['seq0'] == 40 + M // 2 and t1 == h1['seq0'] == 40 + 2 * L + M // 2
    assert _units(a).tobytes() == filter_blocks(rows, _table(hdr, DMS), NFFT, M, np.complex64, 0, 2).tobytes()
    assert _units(b).tobytes() == filter_blocks(rows, _table(hdr, new), NFFT, M, np.complex64, 2, 3).tobytes()
    assert be.calls.count('chirp') == 2 and be.calls.count('reset') == 1 and be.calls.index('chirp', 3) == 3 + 5
    assert cd.dms == new and cd.stats['dms'] == new and cd.stats['nblock'] == 5


def test_block_plans_at_the_sequence_from_the_header(ring_impl):
    """nfft = overlap = None: cdedisp_plan at the first sequence from the header's band, the largest |DM| and multiple_of; the
    context is made then."""
    hdr = voltage_header(nchan=2, nbeam=2, sfreq=60e6)
    plan = cdedisp_plan(hdr['sfreq'] + CHAN_BW * np.arange(2), CHAN_BW, 4.0, 8)
    assert plan == (512, 136)                                                   # sweep 88 at 60 MHz - half a channel
    rng = np.random.default_rng(4)
    x = gaussian_rows(rng, 2, 2, 1000)
    be = CdedispBackend()
    r1 = Ring("cd-output")
    cd = BeamCoherentDedisperse(LOG, _FakeRing([_FakeSeq(hdr, list(enumerate(_gulps(x, 250))), 2 * 2 * 250 * 8)]), r1, 2, 2, 250, [-4.0], multiple_of=8,
                                backend=be)
    assert be.cd is None
    sink = Sink(r1, 2 * 2 * (512 - 136) * 8)
    sink.start()
    cd.main()
    sink.join(20)
    (hd, _, spans), = sink.sequences
    assert (hd['cdedisp_nfft'], hd['cdedisp_overlap'], hd['cdedisp_dm']) == (512, 136, [-4.0]) and (be.cd['nfft'], be.cd['overlap']) == plan
    assert len(spans) == nblocks_after(1000, 512, 136) == 2


@pytest.mark.parametrize("kw", [dict(nchan=0), dict(ntime_gulp=0), dict(pair0=-1), dict(pair0=2, npair=2), dict(npair=0), dict(dms=[0.1]),
                                dict(dms=[0.1, float('inf')]), dict(dms=None), dict(nfft=300), dict(nfft=128), dict(nfft=1 << 14), dict(overlap=3),
                                dict(overlap=-2), dict(overlap=130), dict(overlap=None), dict(multiple_of=0), dict(multiple_of=7)])
def test_constructor_refuses_bad_arguments(kw):
    be = CdedispBackend()
    with pytest.raises(ValueError, match="BEAM_COHERENT_DEDISPERSE"):
        _block(Ring("a"), Ring("b"), be, **kw)
    assert be.cd is None


@pytest.mark.parametrize("bad", [dict(nchan=4), dict(nbeam=4), dict(nbit=8), dict(complex=False), dict(npol=2), dict(acc_len=32), dict(ntime_sum=4),
                                 dict(nupchan=8), dict(sfreq=None), dict(bw_hz=0.0)])
def test_block_refuses_what_is_not_voltage_beams(bad):
    be = CdedispBackend()
    hdr = voltage_header()
    for k, v in bad.items():
        if v is None:
            del hdr[k]
        else:
            hdr[k] = v
    x = np.zeros((NCHAN, NBEAM, G), np.complex64)
    cd = _block(_FakeRing([_FakeSeq(hdr, [(0, x)], x.nbytes)]), Ring("b"), be)
    with pytest.raises(ValueError, match="BEAM_COHERENT_DEDISPERSE"):
        cd.main()
    assert not [c for c in be.calls if c.startswith('run')]


# ---------------------------------------------------------------- the C entry points
def _gpu_present():
    n = ctypes.c_int(-1)
    return ffi.lib().xengGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


NAMES = ("xengCdedispInitialize", "xengCdedispSetChirp", "xengCdedispRun", "xengCdedispReset", "xengCdedispGetInfo", "xengCdedispCheckGuards",
         "xengCdedispMark", "xengCdedispWait", "xengCdedispTicketDone", "xengCdedispSync", "xengCdedispDestroy")


def test_backend_forwards_every_call_the_block_makes():
    from caltech_bifrost_dsp_amd.backend import HipBackend
    for m in ("cdedisp_initialize", "cdedisp_set_chirp", "cdedisp_run", "cdedisp_reset", "cdedisp_info", "cdedisp_guards_intact", "cdedisp_mark",
              "cdedisp_wait", "cdedisp_sync"):
        assert callable(getattr(HipBackend, m)), m
    for m in ("cdedisp_initialize", "cdedisp_set_chirp", "cdedisp_run", "cdedisp_reset", "cdedisp_mark", "cdedisp_wait", "cdedisp_sync"):
        assert callable(getattr(CdedispBackend, m)), m


def test_entry_points_are_bound_and_check_their_arguments_without_a_gpu():
    """Each new symbol is exported and bound; Run, Reset, Mark and TicketDone are enqueue-only, the calls that wait are not.
    Initialize refuses every size outside the contract before it touches a device; Run refuses null and misaligned pointers, the
    getters null results, SetChirp a null table, before looking for a context; without one, INVALID_STATE."""
    lib = ffi.lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in ffi.SYMBOLS, name
    for name in ("xengCdedispRun", "xengCdedispReset", "xengCdedispMark", "xengCdedispTicketDone"):
        assert name in ffi.ENQUEUE_ONLY, name
    for name in ("xengCdedispInitialize", "xengCdedispSetChirp", "xengCdedispWait", "xengCdedispSync", "xengCdedispCheckGuards", "xengCdedispGetInfo"):
        assert name not in ffi.ENQUEUE_ONLY, name
    # (gpu, nchan, nbeam, ntime, pair0, npair, nfft, overlap)
    good = (0, 96, 32, 480, 0, 16, 4096, 1216)
    for i, v in ((1, 0), (2, 0), (3, 0), (4, -1), (4, 1), (5, 0), (5, 17), (6, 128), (6, 1 << 14), (6, 3000), (7, -2), (7, 1215), (7, 2050), (1, 4000),
                 (3, 1 << 21)):
        args = list(good)
        args[i] = v
        with pytest.raises(ffi.XengError) as ei:
            ffi.call("xengCdedispInitialize", *args)
        assert ei.value.status == INVALID_ARGUMENT, args
    n, s = ctypes.c_longlong(), ctypes.c_int()
    for name, args in (("xengCdedispRun", (None, 4096, ctypes.byref(s))), ("xengCdedispRun", (4096, 4096, None)),
                       ("xengCdedispRun", (4104, 4096, ctypes.byref(s))), ("xengCdedispRun", (4096, 4104, ctypes.byref(s))),
                       ("xengCdedispGetInfo", (None, ctypes.byref(s), ctypes.byref(n), ctypes.byref(n))),
                       ("xengCdedispGetInfo", (ctypes.byref(s), None, ctypes.byref(n), ctypes.byref(n))),
                       ("xengCdedispGetInfo", (ctypes.byref(s), ctypes.byref(s), None, ctypes.byref(n))),
                       ("xengCdedispGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(n), None)),
                       ("xengCdedispSetChirp", (None,)), ("xengCdedispMark", (None,)), ("xengCdedispTicketDone", (1, None)),
                       ("xengCdedispCheckGuards", (None,))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_ARGUMENT, (name, args)
    if _gpu_present():
        return                      # (a context may be live in this process; tests/test_cdedisp_gpu.py covers the rest)
    t = ctypes.c_ulonglong()
    f = np.zeros(4, np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for name, args in (("xengCdedispRun", (4096, 4096, ctypes.byref(s))), ("xengCdedispRun", (4096, None, ctypes.byref(s))), ("xengCdedispReset", ()),
                       ("xengCdedispSetChirp", (f,)), ("xengCdedispGetInfo", (ctypes.byref(s), ctypes.byref(s), ctypes.byref(n), ctypes.byref(n))),
                       ("xengCdedispMark", (ctypes.byref(t),)), ("xengCdedispWait", (1,)), ("xengCdedispTicketDone", (1, ctypes.byref(s))),
                       ("xengCdedispSync", ()), ("xengCdedispCheckGuards", (ctypes.byref(s),))):
        with pytest.raises(ffi.XengError) as ei:
            ffi.call(name, *args)
        assert ei.value.status == INVALID_STATE, name
    ffi.call("xengCdedispDestroy")      # (nothing to destroy: success)
