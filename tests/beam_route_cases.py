"""Constructed weights and voltages on both sides of every threshold of the beamformer's precision control
(csrc/beamform_kernels.h, "precision of the fixed-point weights"), shared by tests/test_beam_route_cpu.py (the rule's
restatement and its CPU emulation) and tests/test_beamform_rows_gpu.py (the device)."""
import numpy as np

NTIME, NCHAN, NINPUT, NBEAM = 130, 2, 192, 34     # two work-groups (ragged), three 64-input chunks, a full + a ragged tile


def block_weights(nchan, nbeam, ninput, sfreq=50e6, chan_bw=23925.78125, seed=0xaabbccdd):
    """Weights as the Beamform block builds them (beamform_block.py:343-350) from the test's random delays / amps / cal gains
    (beamformer_test.py:131-139)."""
    rng = np.random.default_rng(seed)
    freqs = sfreq + np.arange(nchan) * chan_bw
    w = np.zeros((nchan, nbeam, ninput), np.complex64)
    for b in range(nbeam):
        delays_ns = rng.uniform(0, 12, ninput)
        amps = rng.uniform(10, 17, ninput)
        cal = (rng.uniform(-1, 1, (nchan, ninput)) + 1j * rng.uniform(-1, 1, (nchan, ninput))).astype(np.complex64)
        w[:, b, :] = amps * np.exp(1j * 2 * np.pi * freqs[:, None] * delays_ns * 1e-9) * cal
    return w


def voltages(rng, ntime, nchan, ninput, dead=()):
    vin = rng.integers(0, 256, (ntime, nchan, ninput), dtype=np.uint8)
    vin[:, :, list(dead)] = 0
    return vin


def one_binade_weights(rng, nchan, nbeam, ninput):
    """Every entry's max(|re|, |im|) in [1, 2): one exponent bucket, so a power of two moves an entry by whole buckets."""
    big = rng.uniform(1, 2, (nchan, nbeam, ninput))
    small = rng.uniform(-1, 1, (nchan, nbeam, ninput)) * big
    swap = rng.random((nchan, nbeam, ninput)) < 0.5
    sign = rng.choice([-1.0, 1.0], (nchan, nbeam, ninput))
    return (np.where(swap, small, big * sign) + 1j * np.where(swap, big * sign, small)).astype(np.complex64)


THRESHOLDS = {          # name: totals (tiles_bf16, outlier_inputs) of the single-tile context, member 0 and member 1
    "row_out": ((0, 8), (1, 0)),        # BI_ROW_OUT: 8 against 9 dominant weights (x 2^12) in a row
    "tile_out": ((0, 32), (1, 0)),      # BI_TILE_OUT: 32 against 33 distinct dominant inputs in a tile
    "gap": ((0, 0), (0, 1)),            # BI_GAP_BINADES: one entry x 2^3 (top of the row) against x 2^4 (an outlier)
    "guard": ((0, 0), (1, 0)),          # BI_GUARD_BINADES: 9 entries x 2^4 above the rest against x 2^5
    "spread": ((0, 0), (1, 0)),         # BI_SPREAD_BINADES: 60 % of a row's entries x 2^3 above the rest against x 2^4
    "share": ((0, 0), (1, 0)),          # BI_LOW_NUM / BI_LOW_DEN: 7/8 of a row's entries x 2^6 against one entry fewer
}


def apply_threshold(name, member, rows, idx):
    """Edit rows [>= 5][ninput] (a view into one tile's weights) in place; idx: distinct inputs.  Returns the inputs to kill."""
    big = np.float32(4096.0)
    if name == "row_out":
        rows[1, idx[:8 + member]] *= big
        return idx[:8 + member]
    if name == "tile_out":
        for r in range(4):
            rows[r, idx[8 * r:8 * r + 8]] *= big
        if member:
            rows[4, idx[32]] *= big
        return idx[:33]
    if name == "gap":
        rows[2, idx[0]] *= np.float32(2.0 ** (3 + member))
        return idx[:0]
    if name == "guard":
        rows[3, idx[:9]] *= np.float32(2.0 ** (4 + member))
        return idx[:9]
    ninput = rows.shape[1]
    if name == "spread":                # the median sits among the dominant entries, the lower eighth among the rest
        k = (3 * ninput) // 5
        rows[0, idx[:k]] *= np.float32(2.0 ** (3 + member))
        return idx[:k]
    if name == "share":                 # exactly 7/8 dominant: the lower-eighth entry is one of them and nothing is routed
        assert ninput % 8 == 0          # (live inputs: past 7/8 the rule does not protect weights on the minority alone)
        rows[4, idx[:7 * ninput // 8 - member]] *= np.float32(64.0)
        return idx[:0]
    raise ValueError(name)


def threshold_case(name, member, multi=False, ninput=NINPUT):
    """-> (vin, w, expected single-tile totals or None).  multi: three channels, two tiles (40 beams): member `member` in
    (channel 0, tile 0) and the other member in (channel 2, tile 1); every other tile keeps plain rows."""
    rng = np.random.default_rng(sum(name.encode()) + 2 * member + multi)
    idx = rng.permutation(ninput)
    if not multi:
        w = one_binade_weights(rng, 1, 8, ninput)
        dead = apply_threshold(name, member, w[0], idx)
        return voltages(rng, NTIME, 1, ninput, dead), w, THRESHOLDS[name][member]
    w = one_binade_weights(rng, 3, 40, ninput)
    dead = list(apply_threshold(name, member, w[0, :32], idx)) + list(apply_threshold(name, 1 - member, w[2, 32:], idx))
    return voltages(rng, NTIME, 3, ninput, dead), w, None


EXTRAS = ["shared_outlier", "last_input", "ragged_chunk", "bucket0"]


def extra_case(name):
    """-> (vin, w, expected single-tile totals).  Dominant weights sit on LIVE inputs here: a wrong entry of the tile's
    outlier table would show in the output."""
    rng = np.random.default_rng(sum(name.encode()))
    big = np.float32(4096.0)
    ninput = 48 if name == "ragged_chunk" else NINPUT
    w = one_binade_weights(rng, 1, 6, ninput)
    if name == "shared_outlier":        # rows 0, 2, 4 list input 7, rows 1, 3 input 9, row 5 nothing
        w[0, 0::2, 7] *= big
        w[0, 1:5:2, 9] *= big
        tot = (0, 2)
    elif name == "last_input":
        w[0, 1, ninput - 1] *= big
        w[0, 4, 0] *= big
        tot = (0, 2)
    elif name == "ragged_chunk":        # 48 inputs: one chunk of 64 with 16 padded columns; outliers in its second K step
        w[0, 0, 47] *= big
        w[0, 3, 40] *= big
        w[0, 3, 32] *= big
        tot = (0, 3)
    elif name == "bucket0":             # zeros and denormals: exponent field 0
        w[0, 0, 0::3] = 0
        w[0, 1, 1::4] = np.complex64(1e-40 + 1e-40j)
        keep = w[0, 2, [5, 77, 130, 191]].copy()
        w[0, 2] = 0
        w[0, 2, [5, 77, 130, 191]] = keep * np.array([1, 1, 1, big], np.complex64)
        w[0, 3] = 0
        w[0, 4, 10:40] = np.complex64(3e-39j)
        w[0, 4, 100] *= big
        tot = (0, 5)                    # row 2's four entries all stand out of its zeros; row 4's input 100
    else:
        raise ValueError(name)
    return voltages(rng, NTIME, 1, ninput), w, tot


UNEVEN = ["per_beam", "per_channel", "checkerboard", "zero_rows"]


def uneven_case(name, ninput=NINPUT):
    """Rows of one tile, or channels, on very different scales.  -> (vin, w)"""
    rng = np.random.default_rng(sum(name.encode()) + ninput)
    w = block_weights(NCHAN, NBEAM, ninput)
    dead = []
    if name == "per_beam":
        w *= (10.0 ** rng.uniform(-6, 6, (1, NBEAM, 1))).astype(np.float32)
    elif name == "per_channel":
        w *= (10.0 ** rng.uniform(-6, 6, (NCHAN, 1, 1))).astype(np.float32)
    elif name == "checkerboard":        # neighbours in a tile, and the same beam in the next channel, differ by 1e8
        sign = (np.arange(NCHAN)[:, None] + np.arange(NBEAM)[None, :]) % 2
        w *= np.where(sign, 1e4, 1e-4).astype(np.float32)[:, :, None]
    elif name == "zero_rows":           # an all-zero row between live rows; a row with weights on dead inputs only
        dead = list(rng.choice(ninput, 20, replace=False))
        w[:, 3] = 0
        w[:, 33] = 0
        live = np.ones(ninput, bool)
        live[dead] = False
        w[:, 5, live] = 0
        w[:, 32, live] = 0
        w[0, 5, dead[:4]] *= np.float32(1e3)
    else:
        raise ValueError(name)
    vin = voltages(rng, NTIME, NCHAN, ninput, dead)
    if name == "zero_rows":             # imaginary -1 on the live inputs of some samples: the zero digits of rows 5 and 32
        live_idx = np.flatnonzero(live)  # meet ~xi = 0 there and -16 on the dead inputs; the wsum offset cancels it exactly
        vin[np.ix_(np.arange(0, NTIME, 3), np.arange(NCHAN), live_idx)] = 0x0F
    return vin, w


TAIL_SEEDS = 24         # sigma 0.5, 2 or 4 by seed: in these, sigma 0.5 routes nothing and sigma 2 and 4 route every tile
MIXED_SEEDS = 8         # ... so eight more, with a sigma per row and a few stand-out entries: outliers and partial routing


def heavy_tail_case(seed, ninput=NINPUT, nbeam=NBEAM):
    """Log-normal magnitudes inside every row, a random 0..60 % of the inputs dead.  Seeds below TAIL_SEEDS: one sigma (0.5,
    2 or 4 by seed).  The seeds after them: a sigma per (channel, beam) row from 0.2 to 0.8, in a third of the rows one to
    three entries x 2^12, and in one row of forty 55 to 85 % of the entries x 2^2 .. 2^5."""
    rng = np.random.default_rng(1000 + seed)
    w = block_weights(NCHAN, nbeam, ninput, seed=seed + 1)
    if seed < TAIL_SEEDS:
        sigma = (0.5, 2.0, 4.0)[seed % 3]
    else:
        sigma = rng.uniform(0.2, 0.8, (NCHAN, nbeam, 1))
        for c, b in zip(*np.nonzero(rng.random((NCHAN, nbeam)) < 1 / 3)):
            w[c, b, rng.choice(ninput, rng.integers(1, 4), replace=False)] *= np.float32(4096.0)
        for c, b in zip(*np.nonzero(rng.random((NCHAN, nbeam)) < 1 / 40)):
            k = int(rng.uniform(0.55, 0.85) * ninput)
            w[c, b, rng.choice(ninput, k, replace=False)] *= np.float32(2.0 ** rng.integers(2, 6))
    w = (w * np.exp(sigma * rng.standard_normal(w.shape))).astype(np.complex64)
    dead = rng.choice(ninput, int(rng.uniform(0, 0.6) * ninput), replace=False)
    return voltages(rng, NTIME, NCHAN, ninput, dead), w


MAJORITY = [(ninput, share, gain) for ninput in (192, 704) for share in (0.52, 0.80) for gain in (64.0, 1e3)]


def majority_case(ninput, share, gain):
    """Dominant weights on MOST of the inputs, all of them dead: the ordinary minority alone makes the output."""
    rng = np.random.default_rng(int(ninput + 100 * share + gain))
    w = block_weights(NCHAN, NBEAM, ninput)
    dead = rng.choice(ninput, int(round(share * ninput)), replace=False)
    w[:, :, dead] *= np.float32(gain)
    return voltages(rng, NTIME, NCHAN, ninput, dead), w
