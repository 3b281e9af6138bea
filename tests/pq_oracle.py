"""TEST HELPER — numpy restatement of the product-quantisation k-means contract of qcnn_quantize_layer (include/qcnn_hip.h,
DESIGN.md "Quantising dense weights"), bit for bit.

float32 numpy element-wise operations round once each and never contract into FMA, so ``t = p - c; d = d + t * t`` is
the contract's distance.  ``np.bincount(.., weights=fp64)`` adds in array order: the ascending-n fp64 member sums.
Sub-spaces are processed in chunks (memory stays bounded); a sub-space whose assignments stopped changing is a fixed point
of the update, so running it along with the others changes none of its bits.
"""
from __future__ import annotations

import numpy as np

CHUNK_FLOATS = 1 << 24        # float32 distance entries [mc][N][K] per chunk (64 MB)


def layer_dims(w):
    w = np.asarray(w)
    if w.ndim == 4:
        ct, cin, kh, kw = w.shape
    else:
        (ct, cin), kh, kw = w.shape, 1, 1
    return ct, cin, kh * kw


def points(w, M, Cs):
    """[M][N][Cs] float32, point n = ct * taps + t, dims >= CsEff zero."""
    ct, cin, taps = layer_dims(w)
    w3 = np.asarray(w, np.float32).reshape(ct, cin, taps)
    pad = np.zeros((ct, M * Cs, taps), np.float32)
    pad[:, :cin] = w3
    return np.ascontiguousarray(pad.reshape(ct, M, Cs, taps).transpose(1, 0, 3, 2).reshape(M, ct * taps, Cs))


def cs_eff(cin, M, Cs):
    return [min(cin - m * Cs, Cs) for m in range(M)]


def dist(p, c, cse):
    """p [..., N, Cs], c [..., K, Cs] -> [..., N, K] float32, dims j < cse in order."""
    d = np.zeros(p.shape[:-1] + (c.shape[-2],), np.float32)
    for j in range(cse):
        t = p[..., :, None, j] - c[..., None, :, j]
        d = d + t * t
    return d


def assign(p, c, cse):
    d = dist(p, c, cse)
    a = np.argmin(d, axis=-1)                                   # first minimum: lowest k
    return a, np.take_along_axis(d, a[..., None], axis=-1)[..., 0]


def update(p, c, a, cse):
    """p [mc][N][Cs], c [mc][K][Cs], a [mc][N] -> new c."""
    mc, n, _ = p.shape
    K = c.shape[1]
    idx = (np.arange(mc)[:, None] * K + a).reshape(-1)
    cnt = np.bincount(idx, minlength=mc * K).reshape(mc, K)
    out = c.copy()
    for j in range(cse):
        s = np.bincount(idx, weights=p[:, :, j].reshape(-1).astype(np.float64), minlength=mc * K).reshape(mc, K)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = (s / cnt).astype(np.float32)
        out[:, :, j] = np.where(cnt > 0, v, c[:, :, j])
    return out


def seed(p, K, cse):
    """Farthest-first code books of sub-spaces p [..., N, Cs] -> [..., K, Cs]."""
    lead = p.shape[:-2]
    q = p.reshape((-1,) + p.shape[-2:])
    r = np.arange(q.shape[0])
    c = np.zeros((q.shape[0], K, q.shape[2]), np.float32)
    c[:, 0] = q[:, 0]
    dmin = dist(q, c[:, 0:1], cse)[..., 0]
    for i in range(1, K):
        n = np.argmax(dmin, axis=1)                             # first maximum: lowest n
        c[:, i] = q[r, n]
        if i < K - 1:
            dmin = np.minimum(dmin, dist(q, c[:, i:i + 1], cse)[..., 0])
    return c.reshape(lead + (K, q.shape[2]))


def quantize_layer(w, M, K, Cs, ctrd_init=None, max_iter=30):
    """(ctrd [M][K][Cs], asmt in file order, stats dict(sse_init, sse, iters, unconverged)) of the contract."""
    ct, cin, taps = layer_dims(w)
    P = points(w, M, Cs)
    N = P.shape[1]
    cses = cs_eff(cin, M, Cs)
    C = np.zeros((M, K, Cs), np.float32)
    A = np.zeros((M, N), np.int64)
    sse0 = sse1 = 0.0
    steps_max, unconv = 0, 0
    mc_max = max(1, CHUNK_FLOATS // max(1, N * K))
    full = M if cses[-1] == Cs else M - 1                       # a partial last sub-space is a chunk of its own
    chunks = [(m0, min(full, m0 + mc_max)) for m0 in range(0, full, mc_max)] + ([(M - 1, M)] if full < M else [])
    for m0, m1 in chunks:
        cse = cses[m0]
        p = P[m0:m1]
        if ctrd_init is not None:
            c = np.array(ctrd_init, np.float32)[m0:m1].copy()
        else:
            c = seed(p, K, cse)
        a, dm = assign(p, c, cse)
        sse0 += float(dm.astype(np.float64).sum())
        changing = np.zeros(m1 - m0, bool)
        steps = 0
        for _ in range(max_iter):
            c = update(p, c, a, cse)
            a2, dm = assign(p, c, cse)
            steps += 1
            changing = (a2 != a).any(axis=1)
            a = a2
            if not changing.any():
                break
        steps_max = max(steps_max, steps)
        if steps == max_iter:
            unconv += int(changing.sum())
        sse1 += float(dm.astype(np.float64).sum())
        c[:, :, cse:] = 0.0
        C[m0:m1], A[m0:m1] = c, a
    w = np.asarray(w)
    ashape = (ct, M) if w.ndim == 2 else (ct,) + w.shape[2:] + (M,)
    asmt = np.ascontiguousarray(A.T).astype(np.uint8).reshape(ashape)
    return C, asmt, dict(sse_init=sse0, sse=sse1, iters=steps_max, unconverged=unconv)


class OracleEngine:
    """quantize_layer of QcnnEngine's signature, computed by this module (CPU tests of the Python layer above the engine)."""

    def quantize_layer(self, weights, M, K, Cs, ctrd_init=None, max_iter=30):
        return quantize_layer(weights, M, K, Cs, ctrd_init=ctrd_init, max_iter=max_iter)
