"""The beamformer on two-part packet slabs whose parts split a wave and are of different kinds (xengBeamformRunSlabs).

The ABI takes a first part of any multiple of 16 samples.  The int8x3 kernel stages 16 rows per LDS-DMA piece, the bf16x3 kernel 32
rows: a split at 16 mod 32 puts lanes 0..31 and 32..63 of one of its waves into different parts, and the two parts may be read in
different ways -- one through its packet index (descriptor pad 2), the other as the scratch gulp it was scattered into (pad 1: a
valid packet of another geometry, or a part that the index pass cannot take, such as an empty one).  The bf16x3 kernel once took the
way from lane 0 for the whole wave; it selects per lane.

Geometry: 64 stands (two 64-input blocks per sample), 4 channels (the plain block mapping), 32 beams, 224 = 128 + 96 samples (the last
work-group tile is partial), an outlier input on every row and channel 0 routed to the bf16x3 kernel (tests/slab_parts._beam_weights).
Splits 16, 80, 144, 208 (16 mod 32: inside the first wave, a middle wave, the second tile's first wave, 16 samples before the end) and
96 (0 mod 32, the control).  Part kinds R, L, F, E: tests/slab_parts.part_packets.

Reference: xengBeamformRunVersioned on what oracle.snap2_unpack makes of the packets -- the same kernels do the arithmetic, only the
addresses differ, so the outputs are compared bit for bit (that beamformer is held against float64 in tests/test_beamform_gpu.py and
tests/test_beamform_rows_gpu.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import xeng_oracle as orc  # noqa: E402,F401
from tests import input_pins  # noqa: E402
from tests.slab_parts import SEQ0, CHAN0, _slab, _beam_init, _beam_weights, gpu, part_gulp, part_packets, voltages  # noqa: E402,F401

NSTAND, NCHAN, NTIME, NBEAM = 64, 4, 224, 32
NINPUT = NSTAND * 2
SPLITS = (16, 80, 144, 208, 96)
PAIRS = (("L", "F"), ("F", "L"), ("R", "F"), ("F", "R"), ("L", "L"), ("F", "F"), ("L", "E"), ("E", "L"), ("R", "R"))
CONTEXTS = [("", "1"), ("bf16x3", "1"), ("", None), ("bf16x3", None), ("", "0"), ("bf16x3", "0"), ("f32", None)]
GUARD = 4096


@pytest.fixture(scope="module")
def cases():
    """computed once, shared by the seven contexts and left unchanged: per (split, side, kind) the slab bytes and the unpacked part"""
    vin = voltages(NTIME, NCHAN, NSTAND, seed=224)
    stride = 32 + NCHAN * 64
    parts = {}
    for split in SPLITS:
        for side, (lo, hi) in enumerate(((0, split), (split, NTIME))):
            for kind in "RLFE":
                pk, _ = part_packets(kind, vin, lo, hi, seed=side)
                raw = _slab(pk)[0] if pk else np.zeros(stride, dtype=np.uint8)      # (E: npkt = 0 with a valid pointer)
                assert not pk or _slab(pk)[1] == stride
                assert len(pk) <= 448
                parts[split, side, kind] = (raw, len(pk), part_gulp(pk, lo, hi, NCHAN, NINPUT))
    w = _beam_weights(np.random.default_rng(224), NCHAN, NBEAM, NINPUT)
    return parts, w, stride


def _expected_counts(mode, tables, kinds, by_index):
    """(nscattered, nirregular) of one call, from slab.hip and run_slabs:
    by strides (XENG_SLAB_TABLES=0, the fp32 kernel -- run_slabs creates no packet index for it --, and the default context until a
      part was not regular): slab_prepare_kernel sends every part that is not a regular slab to the scratch gulp, `fallbacks` += 1 --
      L and F by their packet count (slab_maybe_regular; a count that happened to fit would fail the per-packet check), E by npkt > 0
      of slab_maybe_regular (force_scratch);
    by index (XENG_SLAB_TABLES=1; the default context from the call after the first irregular part on): slab_index_prepare_kernel
      gives L its index (pad 2) and `irregular` += 1 as not every (sample, block) sits in its slot; F has a valid packet of another
      geometry (`other`) -> scratch, `fallbacks` += 1; E fails npkt > 0 of slab_index_prep_ok -> force_scratch -> scratch,
      `fallbacks` += 1; R gets its index and is counted nowhere."""
    if by_index:
        return sum(k in "FE" for k in kinds), sum(k == "L" for k in kinds)
    return sum(k != "R" for k in kinds), 0


@pytest.mark.parametrize("mode,tables", CONTEXTS)
def test_parts_that_split_a_wave_in_every_mix_of_kinds(gpu, cases, mode, tables):
    """every (split, pair) in one context, 45 consecutive calls: the beams of the two slabs equal, bit for bit, those of the unpacked
    gulp; the guard band behind the output is untouched; the counters are what slab.hip gives (see _expected_counts).

    Before the per-lane selection the bf16x3 kernel (channel 0's tiles in the default route, every tile under XENG_BEAM=bf16x3) misread
    in the contexts that follow the indices, at each split s = 16 mod 32, the wave that stages rows s - 16 .. s + 15: lanes 32..63 (rows
    s .. s + 15, part 1) took part 0's way.  (L,F), (L,E): lanes 32..63 read scratch voltage bytes as index entries; (F,L), (E,L): lanes
    32..63 added (i >> 6) * packet_stride to an index row's address; (R,F), (F,R): the same two with a regular part 0 / part 1 by
    index.  (L,L), (F,F), (R,R) and the split at 96 were right before and are the controls."""
    ffi = gpu.ffi
    parts, w, stride = cases
    _beam_init(ffi, mode, NINPUT, NCHAN, NTIME, NBEAM, tables=tables)
    nout = NCHAN * NBEAM * NTIME * 8
    wpin = input_pins.upload("weights", ffi.DeviceBuffer(w.nbytes), w)
    dw = wpin.buf
    o1, o2 = ffi.DeviceBuffer(nout), ffi.DeviceBuffer(nout + GUARD)
    dfull = ffi.DeviceBuffer(NTIME * NCHAN * NINPUT)
    pin = {key: input_pins.upload("part %d of split %d, kind %s" % (key[1], key[0], key[2]), ffi.DeviceBuffer(raw.size), raw)
           for key, (raw, _, _) in parts.items()}
    dev = {key: p.buf for key, p in pin.items()}
    index_next = tables == "1" and mode != "f32"             # (the default context goes over to the indices once a part was not regular)
    seen_loss_matter = False
    ncall = 0
    try:
        for split in SPLITS:
            outs = {}
            for pair in PAIRS:
                (_, n0, g0), (_, n1, g1) = parts[split, 0, pair[0]], parts[split, 1, pair[1]]
                unpacked = np.concatenate([g0, g1])
                assert unpacked.shape == (NTIME, NCHAN, NINPUT)
                full_pin = input_pins.upload("unpacked gulp", dfull, unpacked.reshape(-1))
                ffi.call("xengMemset", o2.ptr, 0x5A, o2.nbytes)
                ffi.call("xengBeamformRunVersioned", dfull.ptr, o1.ptr, dw.ptr, 1)
                ffi.call("xengBeamformRunSlabs", dev[split, 0, pair[0]].ptr, n0, split, dev[split, 1, pair[1]].ptr, n1, stride, SEQ0, CHAN0,
                         o2.ptr, dw.ptr, 1)
                ffi.call("xengBeamformSync")
                ns, ni = ctypes.c_int(-1), ctypes.c_int(-1)
                ffi.call("xengBeamformGetSlabStats", ctypes.byref(ns), ctypes.byref(ni))
                a, b = o1.download(np.uint32), o2.download(np.uint32)
                tag = (mode, tables, split, pair, ncall)
                for p in (full_pin, wpin, pin[split, 0, pair[0]], pin[split, 1, pair[1]]):      # what this call was given
                    p.check()
                assert np.all(b[nout // 4:] == 0x5A5A5A5A), ("guard band", tag)
                nbad = int(np.count_nonzero(a != b[:nout // 4]))
                print("beam slab parts", tag, "words that differ:", nbad, "counters:", (ns.value, ni.value))
                assert np.array_equal(a, b[:nout // 4]), tag
                nonreg = sum(k != "R" for k in pair)
                assert (ns.value, ni.value) == _expected_counts(mode, tables, pair, index_next), (tag, ns.value, ni.value)
                if tables is None:
                    assert ns.value + ni.value == nonreg, (tag, ns.value, ni.value)
                    index_next = index_next or (mode != "f32" and nonreg > 0)
                outs[pair] = a
                ncall += 1
            if not (np.array_equal(outs["L", "F"], outs["R", "R"]) and np.array_equal(outs["F", "L"], outs["R", "R"])):
                seen_loss_matter = True
        assert seen_loss_matter, "the losses changed no beam: the comparison would pass with the parts ignored"
        assert ncall == len(SPLITS) * len(PAIRS)
        for p in pin.values():                               # ... and every part once more: no call wrote into another call's part
            p.check()
    finally:
        ffi.call("xengBeamformDestroy")
        for d in list(dev.values()) + [dw, o1, o2, dfull]:
            d.free()
