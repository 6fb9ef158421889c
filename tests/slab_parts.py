"""Packet slabs for the slab tests: the constants and small helpers that tests/test_slab_gpu.py and
tests/test_beam_slab_parts_gpu.py share, and the four kinds of gulp part that the beamformer's two-part calls are run on.
Nothing here needs a GPU: tests/test_oracle.py checks on the CPU what the oracle's unpacker makes of each kind."""
import numpy as np
import pytest

from oracle import xeng_oracle as orc

SEQ0, CHAN0 = 10 ** 12 + 7, 1000


@pytest.fixture(scope="module")
def gpu():
    """the GPU tests' driver module (imported by the test modules that use it)"""
    from tests import gpu_util
    assert gpu_util.ffi.device_count() >= 1
    return gpu_util


def _slab(pkts):
    stride = len(pkts[0])
    assert all(len(p) == stride for p in pkts)
    return np.frombuffer(b"".join(pkts), dtype=np.uint8), stride


def _beam_init(ffi, mode, ninput, nchan, ntime, nbeam, ntime_blocks=0, tables=None):
    """tables: XENG_SLAB_TABLES for this context ("1": the parts are read through their packet indices from the first call on)"""
    import os
    old = {k: os.environ.pop(k, None) for k in ("XENG_BEAM", "XENG_SLAB_TABLES")}
    if mode:
        os.environ["XENG_BEAM"] = mode
    if tables is not None:
        os.environ["XENG_SLAB_TABLES"] = tables
    try:
        ffi.call("xengBeamformInitialize", 0, ninput, nchan, ntime, nbeam, ntime_blocks)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _beam_weights(rng, nchan, nbeam, ninput):
    w = (rng.uniform(-17, 17, (nchan, nbeam, ninput)) + 1j * rng.uniform(-17, 17, (nchan, nbeam, ninput))).astype(np.complex64)
    w[:, :, 3] *= 4096.0                                                       # an outlier input on every row
    w[0] *= np.exp(rng.uniform(-12, 12, (nbeam, ninput))).astype(np.float32)    # channel 0: routed to the bf16x3 kernel
    return w


def voltages(ntime, nchan, nstand, seed):
    """u8[ntime][nchan][nstand][2], all 256 byte values (tests/gpu_util.synth_voltages 'full')"""
    return np.random.RandomState(seed).randint(0, 256, size=(ntime, nchan, nstand, 2), dtype=np.uint8)


def _packets(v, lo, hi, nstand_per_pkt=32):
    return orc.snap2_packets(v[lo:hi], seq0=SEQ0 + lo, sync_time=1, nchan_blocks=1, nstand_per_pkt=nstand_per_pkt, chan0_pipeline=CHAN0)


def part_packets(kind, vin, lo, hi, seed=0):
    """The packets of samples [lo, hi) of vin (u8[ntime][nchan][nstand][2], 32 stands = 64 inputs per packet) as a gulp part of
    kind
      R  the regular slab
      L  what a lossy link leaves, in arrival order (everything behind a loss one slot early): 2 % of the packets dropped (one at
         least), one whole sample missing, and one (sample, block) carried twice with different payloads -- the voltages' own in its
         place, other ones in a late copy at the end of the slab, which wins
      F  L, and in the middle of the slab one valid in-window packet of another geometry in a slot of the same stride: 16 stands per
         packet, its 128 payload bytes padded with zeros to the slot.  It carries inputs 32..63 of the sample that is otherwise missing,
         so no other packet writes its bytes
      E  no packets
    Returns (packets, info); info names the missing sample, the doubled (sample, block) and the foreign packet (or None)."""
    assert kind in ("R", "L", "F", "E")
    n, nblk = hi - lo, vin.shape[2] * 2 // 64
    if kind == "E":
        return [], {}
    full = _packets(vin, lo, hi)
    if kind == "R":
        return full, {}
    rng = np.random.default_rng([seed, lo, hi])
    other = _packets(vin[::-1], lo, hi)                          # same headers, other payloads
    tmiss = int(rng.integers(n))
    tdup = int((tmiss + 1 + rng.integers(n - 1)) % n)
    bdup = int(rng.integers(nblk))
    keep = [i for i in range(len(full)) if i // nblk != tmiss]
    cand = [i for i in keep if i != tdup * nblk + bdup]
    lost = set(rng.choice(cand, size=max(1, round(0.02 * len(full))), replace=False).tolist())
    pk = [full[i] for i in keep if i not in lost]
    late = other[tdup * nblk + bdup]
    assert late != full[tdup * nblk + bdup] and late[:32] == full[tdup * nblk + bdup][:32]
    pk.append(late)
    info = {"tmiss": tmiss, "dup": (tdup, bdup), "foreign": None, "nlost": len(lost)}
    if kind == "F":
        small = _packets(vin[::-1], lo + tmiss, lo + tmiss + 1, nstand_per_pkt=16)[1]     # inputs 32..63 of that sample
        assert any(small[32:])
        foreign = small + bytes(len(full[0]) - len(small))
        pk.insert(len(pk) // 2, foreign)
        info["foreign"] = foreign
    return pk, info


def part_gulp(pkts, lo, hi, nchan, ninput):
    """what the oracle's unpacker makes of a part: u8[hi - lo][nchan][ninput], missing samples zero, the last packet that carries a
    sample wins, an empty part all zero"""
    return orc.snap2_unpack(pkts, SEQ0 + lo, hi - lo, CHAN0, nchan, ninput)[0]
