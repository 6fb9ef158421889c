"""The contract of xengImage* (include/xeng.h, "Dirty images of the fine-channel visibilities") restated in numpy: float64 by default,
complex64 with a dtype argument (the gap between the two on a test's own inputs is a fifth of that test's bar), the error measure,
a fake backend that serves the image_* calls UpchanImage makes from the restatement, and generators of visibilities."""
import numpy as np

from caltech_bifrost_dsp_amd.blocks.imaging import image_norm
from tests.fake_backend import OracleBackend


def steering(freq, tau, w, dtype=np.complex128):
    """b[c][x][s] = w_s exp(-2 pi i frac(freq[c] tau[x][s])): the product and its fraction of a turn in float64 whatever `dtype`;
    with complex64 the sine, the cosine and the product with w are single precision."""
    turns = np.asarray(freq, np.float64)[:, None, None] * np.asarray(tau, np.float64)[None]
    fr = turns - np.rint(turns)
    if np.dtype(dtype) == np.complex64:
        ang = np.float32(2.0 * np.pi) * fr.astype(np.float32)
        b = (np.cos(ang) - 1j * np.sin(ang)).astype(np.complex64) * np.asarray(w, np.float32)
    else:
        b = np.exp(-2j * np.pi * fr) * np.asarray(w, np.float64)
    assert b.dtype == np.dtype(dtype)
    return b


def masked(V, w, autos):
    """What the kernel loads: V [nfine][nstand][2][nstand][2] with the rows and columns of the stands of weight 0 (and, without
    autos, the 2x2 blocks s = t) replaced by zeros -- a select, so NaN there does not get through."""
    V = np.array(V)
    live = np.asarray(w) != 0
    keep = live[:, None] & live[None, :]
    if not autos:
        keep &= ~np.eye(len(live), dtype=bool)
    return np.where(keep[None, :, None, :, None], V, 0)


def image(V, freq, tau, w, autos, nfavg, dtype=np.complex128):
    """The image f [nfine / nfavg][4][npix] = [XX, YY, Re XY, Im XY] of V complex [nfine][nstand][2][nstand][2]; float64 with
    dtype complex128, float32 (every step of it) with complex64.  norm is image_norm's, float64, applied last."""
    dtype = np.dtype(dtype)
    real = np.float32 if dtype == np.complex64 else np.float64
    nfine, nstand = V.shape[:2]
    Vm = masked(V, w, autos).astype(dtype)
    b = steering(freq, tau, w, dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        I = np.einsum('cxs,cspt,cxt->cpx', np.conj(b), Vm[:, :, [0, 1, 0], :, [0, 1, 1]].transpose(1, 2, 0, 3), b)     # p: XX, YY, XY
    assert I.dtype == dtype
    words = np.stack([I[:, 0].real, I[:, 1].real, I[:, 2].real, I[:, 2].imag], axis=1)                                # [nfine][4][npix]
    with np.errstate(invalid='ignore'):
        grouped = words.reshape(nfine // nfavg, nfavg, 4, -1).sum(axis=1, dtype=real)
    return grouped * real(image_norm(w, autos, nfavg))


def scale(V, w, autos, nfavg):
    """norm * sum_{c in g} sum_{s,t} w_s w_t |V[c][s p][t q]| per (group, word): f64 [nfine / nfavg][4][1], what an error is measured
    against (XY's two words share |V_01|)."""
    nfine = V.shape[0]
    A = np.abs(masked(V, w, autos).astype(np.complex128))
    w = np.asarray(w, np.float64)
    S = np.einsum('s,cspt,t->cp', w, A[:, :, [0, 1, 0, 0], :, [0, 1, 1, 1]].transpose(1, 2, 0, 3), w)                   # [nfine][4]
    return (S.reshape(nfine // nfavg, nfavg, 4).sum(axis=1) * image_norm(w, autos, nfavg))[:, :, None]


def word_error(got, V, freq, tau, w, autos, nfavg, ref=None):
    """|I - I_ref| / scale per word; 0 where both the difference and the scale are 0."""
    ref = image(V, freq, tau, w, autos, nfavg) if ref is None else ref
    d = np.abs(np.asarray(got, np.float64) - ref)
    sc = np.broadcast_to(scale(V, w, autos, nfavg), d.shape)
    return np.where(sc > 0, d / np.where(sc > 0, sc, 1), np.where(d > 0, np.inf, 0.0))


def float_gap(V, freq, tau, w, autos, nfavg):
    """The worst word_error of the complex64 evaluation against the float64 one: a fifth of the float bar."""
    return float(np.max(word_error(image(V, freq, tau, w, autos, nfavg, np.complex64), V, freq, tau, w, autos, nfavg)))


def hermitian_uneven(rng, nfine, nstand, lo=0.5, hi=50.0):
    """Hermitian random matrices whose rows (inputs) have scales of their own between lo and hi: V = D G D with G Hermitian Gaussian
    and D diagonal; complex64 [nfine][nstand][2][nstand][2], Hermitian bit for bit with a real diagonal."""
    n = 2 * nstand
    d = np.exp(rng.uniform(np.log(lo), np.log(hi), (nfine, n)))
    G = rng.standard_normal((nfine, n, n)) + 1j * rng.standard_normal((nfine, n, n))
    G = (G + np.conj(G.transpose(0, 2, 1))) / 2
    V = (d[:, :, None] * G * d[:, None, :]).astype(np.complex64)
    lower = np.tril(np.ones((n, n), bool), -1)
    V = np.where(lower[None], V, 0)
    V = V + np.conj(V.transpose(0, 2, 1)) + np.einsum('ci,ij->cij', (d * d * rng.uniform(0.5, 1.5, (nfine, n))).astype(np.float32), np.eye(n, dtype=np.float32))
    return np.ascontiguousarray(V.astype(np.complex64)).reshape(nfine, nstand, 2, nstand, 2)


def point_source(freq, tau_x0):
    """The visibilities of a unit point source in the direction whose delays are tau_x0 [nstand], the same on both polarisations:
    V[c] = a a^H with a_{s p} = exp(-2 pi i freq[c] tau_x0[s]); complex64 [nfine][nstand][2][nstand][2]."""
    turns = np.asarray(freq, np.float64)[:, None] * np.asarray(tau_x0, np.float64)[None]
    a = np.repeat(np.exp(-2j * np.pi * (turns - np.rint(turns))), 2, axis=1)                 # [nfine][2 nstand]
    V = a[:, :, None] * np.conj(a[:, None, :])
    nfine, nstand = len(freq), len(tau_x0)
    return np.ascontiguousarray(V.astype(np.complex64)).reshape(nfine, nstand, 2, nstand, 2)


def random_array(rng, nstand, extent_m=100.0, height_m=3.0):
    """Stand positions [nstand][3] (east, north, up) in metres: a disc of `extent_m`, heights within +- height_m (non-coplanar)."""
    r = extent_m * np.sqrt(rng.uniform(size=nstand))
    a = rng.uniform(0, 2 * np.pi, nstand)
    return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-height_m, height_m, nstand)], axis=-1)


class ImageBackend(OracleBackend):
    """The oracle backend plus xengImage* served by the complex64 restatement, with the context's state."""

    def __init__(self):
        super().__init__()
        self.im, self.calls = None, []
        self.tau = self.freq = self.w = None

    def image_initialize(self, gpu, nstand, nfine, nfavg, npix):
        if nfine % nfavg:
            return 1
        self.im = dict(nstand=nstand, nfine=nfine, nfavg=nfavg, npix=npix)
        self.tau = self.freq = None
        self.w, self.autos = np.ones(nstand, np.float32), False
        self.calls.append('init')
        return 0

    def image_set_geometry(self, tau, freq):
        u = self.im
        self.tau = np.array(tau, np.float64).reshape(u['npix'], u['nstand'])
        self.freq = np.array(freq, np.float64).reshape(u['nfine'])
        self.calls.append('geometry')
        return 0

    def image_set_weights(self, weights, autos):
        self.w, self.autos = np.array(weights, np.float32).reshape(self.im['nstand']), bool(autos)
        self.calls.append('weights')
        return 0

    def image_run(self, vis_arr, out_arr):
        u = self.im
        if self.tau is None:
            return 2
        V = vis_arr.numpy().reshape(-1).view(np.uint8).view(np.complex64).reshape(u['nfine'], u['nstand'], 2, u['nstand'], 2)
        y = np.ascontiguousarray(image(V, self.freq, self.tau, self.w, self.autos, u['nfavg'], np.complex64), np.float32)
        out_arr.numpy().reshape(-1).view(np.uint8)[:y.nbytes] = y.reshape(-1).view(np.uint8)
        self.calls.append('run')
        return 0

    def image_mark(self):
        return self.beam_mark()

    def image_wait(self, ticket):
        self.beam_wait(ticket)

    def image_sync(self):
        pass
