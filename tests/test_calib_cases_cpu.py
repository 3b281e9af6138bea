"""The crafted cases of the resident calibration (tests/calib_cases.py) and their numpy reference (tests/calib_ref.py), held
to account without a GPU: the reference equals a plain im2col X^T X, every single mistake a kernel could make changes the
result of some case, the "exact" cases are exact in fp32, and the split rule is restated."""
import os
import re

import numpy as np
import pytest

import calib_cases as cc
import calib_ref as cr
from conftest import ROOT

JUNK = 977.5


def all_runs():
    for case in cc.CASES:
        for n in case.ns:
            yield case, n


def maps(case, n):
    x = cc.listed_input(case, cc.images(case, n))
    return x, cr.to_panels(x, JUNK)


def plain_gram(x_nhwc, geom, fc_flatten):
    """X^T X in fp64 by a plain im2col of the NHWC images: zero-padded copies, one slice per tap."""
    x = np.asarray(x_nhwc, np.float64)
    n, H, W, C = x.shape
    if geom["kind"] == "fc":
        X = x.transpose(0, 3, 1, 2).reshape(n, -1) if fc_flatten else x.reshape(n, -1)
        return (X.T @ X)[None]
    grp, k, stride, pad = geom["grp"], geom["k"], geom["stride"], geom["pad"]
    Cg = C // grp
    Ho, Wo = cr.conv_out(H, k, stride, pad), cr.conv_out(W, k, stride, pad)
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    out = []
    for g in range(grp):
        taps = [xp[:, y:y + (Ho - 1) * stride + 1:stride, z:z + (Wo - 1) * stride + 1:stride, g * Cg:(g + 1) * Cg]
                for y in range(k) for z in range(k)]
        X = np.stack(taps, axis=3).reshape(n * Ho * Wo, k * k * Cg)
        out.append(X.T @ X)
    return np.stack(out)


@pytest.mark.parametrize("case,n", list(all_runs()), ids=["%s-n%d" % (c.name, n) for c, n in all_runs()])
def test_reference_equals_plain_im2col(case, n):
    x, panels = maps(case, n)
    geom, flat = cc.geom_of(case)
    got, rows = cr.gram_from_panels(panels, n, geom, flat)
    want = plain_gram(x, geom, flat)
    assert got.shape == want.shape == (geom.get("grp", 1), cr.patch_len(geom), cr.patch_len(geom))
    assert np.array_equal(got, want)                   # integers: every fp64 sum is exact
    assert rows == n * cr.out_pixels(geom)
    assert got.any()


@pytest.mark.parametrize("mistake", cr.MISTAKES)
def test_every_single_mistake_changes_some_case(mistake):
    hit = []
    for case, n in all_runs():
        _, panels = maps(case, n)
        geom, flat = cc.geom_of(case)
        good, _ = cr.gram_from_panels(panels, n, geom, flat)
        bad, _ = cr.gram_from_panels(panels, n, geom, flat, mistake=mistake)
        if not np.array_equal(good, bad):
            hit.append("%s-n%d" % (case.name, n))
    print("%s: changes %s" % (mistake, hit))
    assert hit, "no crafted case would notice: " + mistake


def test_exact_cases_are_exact_in_fp32():
    """A run sums at most 256 products of two map values in fp32: below 2^24 every partial sum is an integer fp32 holds."""
    assert set(cc.EXACT) == {c.name for c in cc.CASES}
    for case, n in all_runs():
        x, _ = maps(case, n)
        assert np.array_equal(x, np.round(x))
        assert float(np.abs(x).max()) ** 2 * 256 < 2 ** 24, case.name
    assert float(np.abs(maps(cc.BY_NAME["second_fc"], 5)[0]).max()) > 3          # interior values, not the inputs' range


def test_split_rule_restated():
    txt = open(os.path.join(ROOT, "quantized-cnn_amd", "csrc", "qcnn_kernels.h")).read()
    run = int(re.search(r"#define\s+QCNN_EC_GRAM_RUN\s+(\d+)", txt).group(1))
    assert run == 2 * cr.PANEL
    geom, _ = cc.geom_of(cc.BY_NAME[cc.SPLITS_CASE])
    panels = (cc.SPLITS_N + cr.PANEL - 1) // cr.PANEL
    assert cr.units_per_split(geom, panels, run) == (2, 35)                       # 70 units, one tile pair: a slab per run
    fc, _ = cc.geom_of(cc.BY_NAME["first_fc"])
    assert cr.units_per_split(fc, 1, run) == (2, 1)                               # one unit: added to the matrix directly
    # AlexNet at a 1000-image batch (8 panels): conv1 fills the chip by splitting, fc6 has tile pairs enough
    conv1 = dict(kind="conv", H=227, W=227, C=3, grp=1, k=11, stride=4, pad=0)
    assert cr.patch_len(conv1) == 363 and cr.units_per_split(conv1, 8, run)[1] == 97
    assert cr.units_per_split(dict(kind="fc", H=6, W=6, C=256), 8, run)[1] == 1
