"""float64 oracle of qcnn_map_diff (include/qcnn_hip.h) and the crafted maps its tests run on.  No GPU, no library.

map_diff(a, b): a (subject) and b (reference) are NHWC maps [n][H][W][C] float32.  A pair is counted when both values are
finite, otherwise it adds 1 to `nonfinite` of its channel and to nothing else; d = (double)a - (double)b; per channel the six
sums in FIELDS order, the total their fold in ascending channel order (max for max_abs_d).  Sums are numpy's by default — exact,
in any order, on the integer maps below — or correctly rounded (math.fsum) with exact_sums=True, which is what a bound on the
device's order of summation is measured against.

Crafted maps:
  integer_map      integers in [-64, 64]: every d, d^2, b^2 and every partial sum of up to 2^20 of them is an integer below 2^53,
                   so all six fields are order-free and the device must return the oracle's bits
  catcher_maps     pairs whose difference needs more than 24 bits — a subtraction made in fp32 rounds it — one kind per channel,
                   so that every channel's sum_d is exact in any order too
  plant            NaN / +Inf / -Inf at chosen (image, element) spots of a or b or both
"""
from __future__ import annotations

import math

import numpy as np

FIELDS = ("count", "nonfinite", "sum_d", "sum_d2", "sum_ref2", "max_abs_d")
I_MAX = FIELDS.index("max_abs_d")
PANEL = 128                      # images per panel of the device layout
INT_MAX_ABS = 64                 # |value| of an integer map
INT_MAX_TERMS = 1 << 20          # pairs per channel up to which the integer maps are promised exact


def _col_sum(x, exact):
    if exact:
        return np.array([math.fsum(x[:, c]) for c in range(x.shape[1])], np.float64)
    return x.sum(axis=0, dtype=np.float64)


def fold(channels):
    """The total of per-channel rows [C][6]: added in ascending channel order in fp64, max for max_abs_d."""
    t = np.zeros(len(FIELDS), np.float64)
    for row in np.asarray(channels, np.float64):
        for j in range(len(FIELDS)):
            t[j] = max(t[j], row[j]) if j == I_MAX else t[j] + row[j]
    return t


def map_diff(a_nhwc, b_nhwc, exact_sums=False):
    """(total float64 [6], channels float64 [C][6]) by the rules of qcnn_map_diff."""
    a = np.asarray(a_nhwc, np.float32)
    b = np.asarray(b_nhwc, np.float32)
    assert a.shape == b.shape and a.ndim == 4
    C = a.shape[-1]
    a64 = a.reshape(-1, C).astype(np.float64)
    b64 = b.reshape(-1, C).astype(np.float64)
    ok = np.isfinite(a64) & np.isfinite(b64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(ok, a64 - b64, 0.0)
        r = np.where(ok, b64, 0.0)
    ch = np.zeros((C, len(FIELDS)), np.float64)
    ch[:, 0] = ok.sum(axis=0)
    ch[:, 1] = (~ok).sum(axis=0)
    ch[:, 2] = _col_sum(d, exact_sums)
    ch[:, 3] = _col_sum(d * d, exact_sums)
    ch[:, 4] = _col_sum(r * r, exact_sums)
    ch[:, 5] = np.abs(d).max(axis=0) if len(d) else 0.0
    return fold(ch), ch


def as_dict(row):
    return {f: float(v) for f, v in zip(FIELDS, row)}


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def bits_equal(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


# ---------------------------------------------------------------------------------------------- crafted maps
def integer_map(shape, seed):
    """[n][H][W][C] float32 of integers in [-64, 64]."""
    return np.random.default_rng(seed).integers(-INT_MAX_ABS, INT_MAX_ABS + 1, shape).astype(np.float32)


def integer_bound(terms_per_channel):
    """The largest value any partial sum of an integer-map field can reach over that many pairs: d^2 <= 128^2."""
    return terms_per_channel * (2 * INT_MAX_ABS) ** 2


def _denormal(k):
    return np.array([k], np.uint32).view(np.float32)[0]


# (a, b): d needs more than 24 bits, so fp32 rounds it: 64 - 3 * 2^-20 to 64, 1 + 2^-23 + 2^-30 to 1 + 2^-23; two denormals one
# ulp apart, whose difference 2^-149 a flush-to-zero subtraction loses
CATCHERS = ((np.float32(64.0), np.float32(3.0 * 2.0 ** -20)),
            (np.float32(1.0 + 2.0 ** -23), np.float32(-(2.0 ** -30))),
            (_denormal(6), _denormal(5)))


def catcher_maps(n, H=4, W=5):
    """(a, b) [n][H][W][3], zero but for one pair per window position (h, w, c): channel c holds CATCHERS[c], in image
    (7 * position) % n, swapped at every third position.  Every channel's sum_d is a sum of equal magnitudes: exact in any order."""
    C = len(CATCHERS)
    a = np.zeros((n, H * W * C), np.float32)
    b = np.zeros_like(a)
    for e in range(H * W * C):
        x, y = CATCHERS[e % C]
        if (e // C) % 3 == 1:
            x, y = y, x
        i = (7 * e) % n
        a[i, e], b[i, e] = x, y
    return a.reshape(n, H, W, C), b.reshape(n, H, W, C)


NONFINITE = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf))


def plant(a, b, spots):
    """Copies of (a, b) with a non-finite value at every spot (image, flat element of the image, 'a' | 'b' | 'both', k):
    NONFINITE[k % 3]; 'both' puts NONFINITE[(k + 1) % 3] into b."""
    a, b = a.copy(), b.copy()
    fa, fb = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    for i, e, where, k in spots:
        if where in ("a", "both"):
            fa[i, e] = NONFINITE[k % 3]
        if where == "b":
            fb[i, e] = NONFINITE[k % 3]
        if where == "both":
            fb[i, e] = NONFINITE[(k + 1) % 3]
    return a, b


def reorder_bounds(a_nhwc, b_nhwc):
    """Per channel and in total, how far an fp64 sum of N terms taken in ANY order can be from the exact sum: N * 2^-52 * sum |x|
    (Higham, Accuracy and Stability, (4.4): (N - 1) u / (1 - (N - 1) u) with u = 2^-53, doubled for the rounding of the
    correctly rounded reference itself and of the products d * d, b * b) — for sum_d2 and sum_ref2, whose terms are >= 0, that is
    N * 2^-52 relative.  Returns (N per channel [C], sum |d| per channel [C])."""
    a = np.asarray(a_nhwc, np.float32)
    C = a.shape[-1]
    a64 = a.reshape(-1, C).astype(np.float64)
    b64 = np.asarray(b_nhwc, np.float32).reshape(-1, C).astype(np.float64)
    ok = np.isfinite(a64) & np.isfinite(b64)
    d = np.where(ok, a64 - b64, 0.0)
    return ok.sum(axis=0).astype(np.float64), np.array([math.fsum(np.abs(d[:, c])) for c in range(C)], np.float64)
