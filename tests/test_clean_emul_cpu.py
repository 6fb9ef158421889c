"""clean_step_kernel without a GPU: the kernel's own source (csrc/clean_kernels.h) compiled as host C++ against a stand-in for
<hip/hip_runtime.h> (tests/clean_emul/) and run by a stand-alone driver as 256 host threads per work-group, launch after launch the
way clean.hip enqueues them, under the address sanitizer.  What this can show is the kernel's logic -- the hand-over of the peak
records and of the stop between launches, the reduction and its ties, the stop rules, the records and the stats, ragged tiles and
ragged stands, the window -- and that no access leaves its buffer; not its arithmetic on the GPU (sincospif is double precision here).

The shapes, the bar and the assertions are those of tests/test_clean_gpu.py's parity test (its first two shapes): the margin of every
peak at least 100 float gaps, the pixels those of the float64 restatement, every word within five times the float32-to-float64 gap of
the restatement on the test's own inputs, per word against max|dirty| + sum_k |C_k|.  Measured here, worst word / bar: 0.20 (22 stands,
37 pixels), 0.20 (35 stands, 300 pixels): the emulated kernel's words are those of the float32 restatement."""
import os
import subprocess

import numpy as np
import pytest

from caltech_bifrost_dsp_amd.blocks.imaging import clean_components, image_norm
from tests.clean_ref import case, clean, component_error, float_gap, peak_margin, scale, word_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "clean_emul")
KERNELS = os.path.join(ROOT, "caltech-bifrost-dsp_amd", "csrc", "clean_kernels.h")
LDS_LINE = "extern __shared__ __attribute__((aligned(16))) uint8_t cln_lds[];"
GAIN = 0.5
SHAPES = [(22, 37, 4, 1, False, 6), (35, 300, 6, 3, True, 8)]       # (nstand, npix, nfine, nfavg, autos, niter), tests/test_clean_gpu.py's


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("clean_emul")
    src = open(KERNELS).read()
    assert src.count(LDS_LINE) == 1
    with open(os.path.join(d, "clean_kernels_host.h"), "w") as f:
        f.write(src.replace(LDS_LINE, "uint8_t* cln_lds = g_lds;"))
    exe = os.path.join(d, "driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address", "-pthread", "-Wno-unknown-pragmas", "-I", str(d),
                           "-I", EMUL, os.path.join(EMUL, "driver.cpp"), "-o", exe])
    return exe, str(d)


def run(driver, dirty, c, niter, gain=GAIN, threshold=0.0, fraction=0.0, mask=None, tau=None):
    exe, d = driver
    tau = c['tau'] if tau is None else tau
    mask = c['mask'] if mask is None else mask
    npix, nstand = tau.shape
    w, autos, nfavg = c['w'], c['autos'], c['nfavg']
    with open(os.path.join(d, "in.bin"), "wb") as f:
        for a, t in ((dirty, np.float32), (c['freq'], np.float64), (tau, np.float64), (w, np.float32), (mask, np.uint8)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    w64 = w.astype(np.float64)
    norm, dsum = np.float32(image_norm(w, autos, nfavg)), np.float32(0.0 if autos else (w64 * w64).sum())
    args = (nstand, len(c['freq']), nfavg, npix, int(autos), niter, repr(float(np.float32(gain))), repr(float(np.float32(threshold))),
            repr(float(np.float32(fraction))), repr(float(norm)), repr(float(dsum)))
    subprocess.check_call([exe] + [str(v) for v in args] + [os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    comps, stats, res = clean_components(np.fromfile(os.path.join(d, "out.bin"), np.uint8), len(c['freq']) // nfavg, niter, npix)
    return res.copy(), comps.copy(), stats.copy()


@pytest.mark.parametrize("nstand,npix,nfine,nfavg,autos,niter", SHAPES)
def test_kernel_source_on_host_threads(driver, nstand, npix, nfine, nfavg, autos, niter):
    """The GPU parity test's assertions; then the prefix property (niter - 1 against niter) and the split property (niter = 2 followed by
    a Run of niter - 2 on its residual) bit for bit."""
    c = case(nstand, npix, nfine, nfavg, autos)
    ref, rcomps, rstats, gaps = clean(c['dirty'], c['freq'], c['tau'], c['w'], autos, nfavg, c['mask'], niter, GAIN)
    sc = scale(c['dirty'], rcomps)
    gap = float_gap(c['dirty'], c['freq'], c['tau'], c['w'], autos, nfavg, ref, rcomps, rstats, GAIN)
    assert peak_margin(gaps, sc) >= 100 * gap, (peak_margin(gaps, sc), gap)
    res, comps, stats = run(driver, c['dirty'], c, niter)
    assert np.array_equal(comps['pixel'], rcomps['pixel']) and np.array_equal(stats['ncomp'], rstats['ncomp']) and np.array_equal(stats['reason'], rstats['reason'])
    err = max(word_error(res, ref, sc).max(), component_error(comps, rcomps, sc).max())
    print("%d stands %d pixels: float32 gap %.2e, bar %.2e, emulated kernel %.2e = %.2f of the bar" % (nstand, npix, gap, 5 * gap, err, err / (5 * gap)))
    assert np.isfinite(res).all() and err <= 5 * gap, (err, 5 * gap)
    assert (comps['pad'] == 0).all() and (stats['pad'] == 0).all() and (stats['ncomp'] == niter).all()
    # stats: |I| of the residual's peak in the window
    I = res[:, 0] + res[:, 1]
    assert np.array_equal(stats['peak'], np.abs(np.where(c['mask'] != 0, I, 0)).max(axis=1))
    # prefix
    res1, comps1, stats1 = run(driver, c['dirty'], c, niter - 1)
    assert comps1.tobytes() == np.ascontiguousarray(comps[:, :niter - 1]).tobytes()
    for g in range(nfine // nfavg):
        x = comps['pixel'][g, niter - 1]
        assert np.array_equal(comps['C'][g, niter - 1], np.float32(GAIN) * res1[g, :, x]) and comps['I'][g, niter - 1] == res1[g, 0, x] + res1[g, 1, x]
    # split
    resa, compsa, _ = run(driver, c['dirty'], c, 2)
    resb, compsb, _ = run(driver, resa, c, niter - 2)
    assert resb.tobytes() == res.tobytes() and np.concatenate([compsa, compsb], axis=1).tobytes() == comps.tobytes()


def test_controls_window_and_a_sub_list(driver):
    """niter = 0 and a threshold above the peak copy the input (reasons 0 and 1); an empty window is reason 2; a NaN group is reason 2
    and leaves the others alone; a sub-list of the pixels that holds the window gives the same words."""
    nstand, npix, nfine, nfavg, autos, niter = SHAPES[1]
    c = case(nstand, npix, nfine, nfavg, autos)
    dirty = c['dirty']
    full = run(driver, dirty, c, 3)
    for kw, reason in ((dict(niter=0), 0), (dict(niter=3, threshold=1e3), 1), (dict(niter=3, mask=np.zeros(npix, np.uint8)), 2)):
        res, comps, stats = run(driver, dirty, c, **kw)
        assert res.tobytes() == dirty.tobytes() and (stats['ncomp'] == 0).all() and (stats['reason'] == reason).all() and (comps['pixel'] == -1).all()
        assert (stats['peak'] == 0).all() if reason == 2 else (stats['peak'] > 0).all()
    bad = dirty.copy()
    bad[1, 0] = np.nan
    res, comps, stats = run(driver, bad, c, 3)
    assert stats['reason'][1] == 2 and res[1].tobytes() == bad[1].tobytes() and res[0].tobytes() == full[0][0].tobytes() and comps[0].tobytes() == full[1][0].tobytes()
    keep = np.flatnonzero((c['mask'] != 0) | (np.arange(npix) % 2 == 0))[5:]
    keep = np.union1d(keep, np.flatnonzero(c['mask']))               # the whole window, about half of the rest, tiles that straddle differently
    res, comps, stats = run(driver, dirty[:, :, keep], c, 3, mask=c['mask'][keep], tau=np.ascontiguousarray(c['tau'][keep]))
    assert len(keep) < npix and res.tobytes() == np.ascontiguousarray(full[0][:, :, keep]).tobytes()
    assert np.array_equal(keep[comps['pixel']], full[1]['pixel']) and comps['C'].tobytes() == full[1]['C'].tobytes() and comps['I'].tobytes() == full[1]['I'].tobytes()
    assert stats.tobytes() == full[2].tobytes()
