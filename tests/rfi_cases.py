"""Input scenes shared by the tests of xengRfi* (tests/test_rfi_emul_cpu.py, tests/test_rfi_gpu.py): seeded noise on a sloped
bandpass with the rows the contract has a rule for planted in it.  Every scene is a fixed function of its arguments."""
import numpy as np

from caltech_bifrost_dsp_amd.blocks import rfi_controls


def scene(seed, nwindows, npair, nfine, nstat, dead_pair=None):
    """f32 [nwindows][npair][nfine][4]: XX and YY of mean b(q), a bandpass falling 10:1 across the band, and sigma 0.1 b(q); cross
    words of sigma 0.07 b(q).  Planted (channels modulo nfine, in pair 0 unless said):
      channel 1: a NaN in word 0 of window 1;  channel 2: a +inf in word 1 of window nstat + 1 (when the scene is that long);
      channel 3: constant (v = 0) in every pair;  pair `dead_pair`: every channel constant (count = 0);
      window nstat // 2: every channel of every pair 2.5 sigma up in XX and YY (a broadband spike: code 2);
      window nstat // 2 + 1: the upper half of the band 40 sigma up (clipped samples; with min_fraction above one half: code 1);
      channel 5: ten times the noise in the second block, pair 0 (an outlier in R there)."""
    rng = np.random.default_rng(seed)
    b = (10.0 ** (-np.arange(nfine) / max(nfine - 1, 1)))[None, None, :, None] * 100.0
    x = rng.standard_normal((nwindows, npair, nfine, 4)) * np.array([0.1, 0.1, 0.07, 0.07]) * b
    x[..., :2] += b
    if nwindows > 2 * nstat - 1:
        x[nstat:2 * nstat, 0, 5 % nfine, :2] = b[0, 0, 5 % nfine, 0] * (1 + rng.standard_normal((nstat, 2)))
    w = nstat // 2
    x[w, :, :, :2] += 0.25 * b[0]
    x[w + 1, :, nfine // 2:, :2] += 4.0 * b[0, :, nfine // 2:]
    x[:, :, 3 % nfine] = b[0, 0, 3 % nfine, 0]
    if dead_pair is not None:
        x[:, dead_pair] = 7.0
    x = x.astype(np.float32)
    x[1, 0, 1 % nfine, 0] = np.nan
    if nwindows > nstat + 1:
        x[nstat + 1, 0, 2 % nfine, 1] = np.inf
    return x


def controls(nfine, zerodm=True, min_fraction=0.6, nsig_chan=4.0):
    return rfi_controls(nsig_chan=nsig_chan, nsig_clip=5.0, nsig_broad=5.0, min_fraction=min_fraction, nfine=nfine) + (int(zerodm),)


def integer_scene(nwindows, nfine):
    """One pair of small integers with the same statistics in many channels: equal R (the tie rule) and mad = 0.  XX = YY = 8 + 2 on
    alternate windows in the even channels, 8 + 4 in channels 1 (mod 4), 8 + 2 with the other phase in channels 3 (mod 4)."""
    n = np.arange(nwindows)[:, None]
    q = np.arange(nfine)[None, :]
    amp = np.where(q % 4 == 1, 4.0, 2.0)
    ph = np.where(q % 4 == 3, 1, 0)
    xx = 8.0 + amp * ((n + ph) % 2)
    x = np.zeros((nwindows, 1, nfine, 4), np.float32)
    x[:, 0, :, 0] = xx
    x[:, 0, :, 1] = xx
    x[:, 0, :, 2] = (n % 3) - 1.0
    return x


# ---------------------------------------------------------------- the planted scene of tests/test_rfi_cpu.py
PLANTED = dict(nwindows=512, nfine=32, nstat=64, burst_chan=9, burst_blocks=(2, 5), dead_chan=20, impulse_at=200, pulse_at=300, sweep=16)


def planted_delays():
    """int [2][nfine]: trial 0 is zero DM, trial 1 a sweep of PLANTED['sweep'] windows from the top channel to the bottom one."""
    q = np.arange(PLANTED['nfine'])
    return np.stack([np.zeros(PLANTED['nfine'], np.int64), np.rint(PLANTED['sweep'] * (PLANTED['nfine'] - 1 - q) / (PLANTED['nfine'] - 1)).astype(np.int64)])


def planted_scene(interference=True, seed=0x5ce9e):
    """f32 [512][1][32][4]: chi-squared noise (100 degrees of freedom: sigma = 0.141 of the mean) on a bandpass falling 10:1, cross
    words of sigma 0.1 of the mean, and a dispersed pulse of 2.5 sigma per channel in XX and YY that reaches the top channel at
    window 300 and the bottom one 16 windows later.  With `interference`: channel 9 bursts to four times its power in a quarter of
    the windows of blocks 2 and 5, channel 20 is dead (zeros), and window 200 carries 3 sigma more in XX and YY of every channel (a
    broadband impulse at zero DM, below the clip in most channels).
    The noise and the pulse are the same with and without."""
    P = PLANTED
    rng = np.random.default_rng(seed)
    nw, nf = P['nwindows'], P['nfine']
    b = 100.0 * 10.0 ** (-np.arange(nf) / (nf - 1.0))
    x = np.empty((nw, 1, nf, 4))
    x[:, 0, :, :2] = rng.chisquare(100, (nw, nf, 2)) / 100.0 * b[None, :, None]
    x[:, 0, :, 2:] = rng.standard_normal((nw, nf, 2)) * 0.1 * b[None, :, None]
    burst = rng.random((len(P['burst_blocks']), P['nstat'])) < 0.25
    sigma = np.sqrt(2.0 / 100.0) * b
    s = planted_delays()[1]
    for q in range(nf):
        x[P['pulse_at'] + s[q], 0, q, :2] += 2.5 * sigma[q]
    if interference:
        for k, blk in enumerate(P['burst_blocks']):
            w = blk * P['nstat'] + np.flatnonzero(burst[k])
            x[w, 0, P['burst_chan'], :2] *= 4.0
        x[:, 0, P['dead_chan']] = 0.0
        x[P['impulse_at'], 0, :, :2] += 3.0 * sigma[:, None]
        x[P['impulse_at'], 0, P['dead_chan']] = 0.0
    return x.astype(np.float32)
