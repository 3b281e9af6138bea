"""Crafted cases of the resident calibration (tests/test_calib_cases_cpu.py, tests/test_gpu_calib_resident.py): the smallest
networks at which each part of k_ec_gram_panel and its engine hook can go wrong.  Values are small integers, so that every
fp32 run sum is exact and the resident matrix must equal the fp64 reference (tests/calib_ref.py) to the bit.

A case: name, in_chw (C, H, W), layers (topology dicts), the listed layer, the batch sizes, the value range of the network
input, and ``weights`` {layer: array} for the layers whose weights matter (all others get zeros; biases are zero).
``listed_input(case, imgs)`` computes the listed layer's INPUT map [n][H][W][C] on the host from the NCHW images."""
import collections
import importlib

import numpy as np

topo = importlib.import_module("quantized-cnn_amd.topology")

Case = collections.namedtuple("Case", "name in_chw layers listed ns lo hi weights")


def _second_fc_weights():
    rng = np.random.default_rng(5)
    return {0: rng.integers(-1, 2, (16, 30)).astype(np.float32)}


CASES = [
    # 5 x 7 x 3, k3 s1 p1 -> P = 27: one diagonal tile; few-image kernels (n = 1, 3), a ragged panel (5), a panel seam (130)
    Case("one_tile", (3, 5, 7), [topo.conv(1, 3, 4, 1, 1)], 0, (1, 3, 5, 130), 0, 3, {}),
    # 9 x 6 x 8, two groups, k3 s2 p0 -> P = 36 per group: the channel offset of a group, stride, a rectangular map
    Case("groups_stride", (8, 9, 6), [topo.conv(0, 3, 4, 2, 2)], 0, (5,), 0, 3, {}),
    # 6 x 5 x 40, k2 s1 p1 -> P = 160: three tiles, off-diagonal pairs, a ragged last tile; three panels
    Case("three_tiles", (40, 6, 5), [topo.conv(1, 2, 4, 1, 1)], 0, (130, 257), 0, 3, {}),
    # 1 x 1 windows on a 3 x 2 map: P exactly at a tile, and one past it
    Case("tile_seam_64", (64, 3, 2), [topo.conv(0, 1, 4, 1, 1)], 0, (5,), 0, 3, {}),
    Case("tile_seam_65", (65, 3, 2), [topo.conv(0, 1, 4, 1, 1)], 0, (5,), 0, 3, {}),
    # 4 x 4 x 2, k5 s1 p2: most taps lie outside the map
    Case("window_over_map", (2, 4, 4), [topo.conv(2, 5, 4, 1, 1)], 0, (5,), 0, 3, {}),
    # an FC layer on the 3 x 2 x 5 (C, H, W) network input: the NCHW flatten with C, H, W > 1
    Case("first_fc", (3, 2, 5), [topo.fcnt(4)], 0, (5,), 0, 3, {}),
    # ... on an interior map: pool 2 x 2 / 2 on 4 x 6 x 5 (H, W, C), the pooled integers flattened
    Case("fc_after_pool", (5, 4, 6), [topo.pool(0, 2, 2), topo.fcnt(4)], 1, (5,), 0, 3, {}),
    # a LATER FC layer reads its map in plain order; interior integers up to 90
    Case("second_fc", (5, 2, 3), [topo.fcnt(16), topo.relu(), topo.fcnt(4)], 2, (5,), 0, 3, _second_fc_weights()),
    # the listed layer's input is fm[1], not fm[0]
    Case("relu_conv", (3, 5, 7), [topo.relu(), topo.conv(1, 3, 4, 1, 1)], 1, (5,), -3, 3, {}),
]
BY_NAME = {c.name: c for c in CASES}
# every case above is exact: max |s|^2 * 256 < 2^24 (the CPU file checks it on the maps themselves)
EXACT = [c.name for c in CASES]
SPLITS_CASE, SPLITS_N = "one_tile", 130          # 2 panels x 35 pixels = 70 units, one tile pair: 35 slabs


def images(case, n, seed=0):
    """[n][C][H][W] float32 integers in [lo, hi]."""
    rng = np.random.default_rng(1000 + seed)
    return rng.integers(case.lo, case.hi + 1, (n,) + tuple(case.in_chw)).astype(np.float32)


def dense_params(case):
    """{layer: dict(bias, weights)} in the convKnl / fcntWei layouts: zeros but for case.weights."""
    sizes = topo.fmap_sizes(case.in_chw, case.layers)
    out = {}
    for i, ly in enumerate(case.layers):
        h, w, c = sizes[i]
        if ly["type"] == topo.CONV:
            shape, ct = (ly["cnt"], c // ly["grp"], ly["knl"], ly["knl"]), ly["cnt"]
        elif ly["type"] == topo.FCNT:
            shape, ct = (ly["nod"], h * w * c), ly["nod"]
        else:
            continue
        wts = np.asarray(case.weights.get(i, np.zeros(shape, np.float32)), np.float32)
        assert wts.shape == shape
        out[i] = dict(bias=np.zeros(ct, np.float32), weights=wts)
    return out


def geom_of(case):
    """(geom dict of calib_ref, fc_flatten) of the listed layer."""
    sizes = topo.fmap_sizes(case.in_chw, case.layers)
    h, w, c = sizes[case.listed]
    ly = case.layers[case.listed]
    if ly["type"] == topo.FCNT:
        first = not any(l["type"] == topo.FCNT for l in case.layers[:case.listed])
        g = dict(kind="fc", H=h, W=w, C=c)
        if not first:
            g["first_fc_hwc"] = sizes[[l["type"] for l in case.layers].index(topo.FCNT)]
        return g, first
    return dict(kind="conv", H=h, W=w, C=c, grp=ly["grp"], k=ly["knl"], stride=ly["stride"], pad=ly["pad"]), False


def listed_input(case, imgs):
    """The listed layer's input map [n][H][W][C] float32, layer by layer on the host (exact: small integers)."""
    x = np.asarray(imgs, np.float32).transpose(0, 2, 3, 1)                      # NHWC
    for i, ly in enumerate(case.layers[:case.listed]):
        t = ly["type"]
        if t == topo.RELU:
            x = np.maximum(x, 0.0)
        elif t == topo.POOL:                                                   # max, ceil mode, windows clipped to the map
            n, h, w, c = x.shape
            k, s, p = ly["knl"], ly["stride"], ly["pad"]
            ho, wo = -(-(h + 2 * p - k) // s) + 1, -(-(w + 2 * p - k) // s) + 1
            y = np.empty((n, ho, wo, c), np.float32)
            for oy in range(ho):
                for ox in range(wo):
                    y0, x0 = max(oy * s - p, 0), max(ox * s - p, 0)
                    y[:, oy, ox] = x[:, y0:min(oy * s - p + k, h), x0:min(ox * s - p + k, w)].max(axis=(1, 2))
            x = y
        elif t == topo.FCNT:                                                   # the reference flattens NCHW
            flat = x.transpose(0, 3, 1, 2).reshape(x.shape[0], -1).astype(np.float64)
            x = (flat @ np.asarray(case.weights[i], np.float64).T).astype(np.float32).reshape(x.shape[0], 1, 1, -1)
        else:
            raise AssertionError("layer type %d in front of a listed layer" % t)
    return np.ascontiguousarray(x)
