"""CPU tier of the error-corrected quantisation: the numpy restatement of the contract (tests/ec_oracle.py) against brute
force and against the k-means oracle, and the case table of the GPU tests."""
import numpy as np
import pytest

import ec_oracle as eo
import pq_oracle


def brute_gram(x, grp, kh, kw, stride, pad):
    n, H, W, C = x.shape
    cg = C // grp
    P = kh * kw * cg
    G = np.zeros((grp, P, P))
    for i in range(n):
        for oy in range((H + 2 * pad - kh) // stride + 1):
            for ox in range((W + 2 * pad - kw) // stride + 1):
                for g in range(grp):
                    s = np.zeros(P)
                    for y in range(kh):
                        for xx in range(kw):
                            iy, ix = oy * stride - pad + y, ox * stride - pad + xx
                            if 0 <= iy < H and 0 <= ix < W:
                                s[(y * kw + xx) * cg:(y * kw + xx + 1) * cg] = x[i, iy, ix, g * cg:(g + 1) * cg]
                    G[g] += np.outer(s, s)
    return G


@pytest.mark.parametrize("shape,grp,k,stride,pad", [((2, 5, 5, 4), 1, 3, 1, 1), ((2, 7, 6, 4), 2, 3, 2, 1), ((3, 4, 4, 6), 2, 1, 1, 0),
                                                    ((1, 9, 9, 2), 1, 5, 2, 0)])
def test_gram_equals_a_brute_force_patch_loop(shape, grp, k, stride, pad):
    x = np.maximum(np.random.default_rng(1).standard_normal(shape), 0).astype(np.float32)
    got, scale = eo.gram(x, grp, k, k, stride, pad)
    want = brute_gram(x.astype(np.float64), grp, k, k, stride, pad)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13) and (scale >= np.abs(got) - 1e-12).all()


def problem(seed, shape, grp, M, K, Cs, n=6, hw=6, stride=1, pad=1):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(shape).astype(np.float32)
    k = shape[2] if len(shape) == 4 else 1
    x = np.maximum(rng.standard_normal((n, hw if k > 1 else 1, hw if k > 1 else 1, shape[1] * grp)) + 0.3, 0).astype(np.float32)
    G = eo.gram(x, grp, k, k, stride, pad if k > 1 else 0)[0]
    ctrd, asmt, st = pq_oracle.quantize_layer(w, M, K, Cs, max_iter=20)
    return w, G, ctrd, asmt, st


def test_identity_objective_is_the_kmeans_sse():
    for shape, M, K, Cs in (((12, 10, 3, 3), 3, 8, 4), ((30, 16), 4, 8, 4)):
        w, _, ctrd, asmt, st = problem(2, shape, 1, M, K, Cs)
        assert abs(eo.objective(w, ctrd, asmt, None) - st["sse"]) <= 1e-6 * st["sse"]       # the SSE sums fp32 distances


@pytest.mark.parametrize("shape,grp,M,K,Cs", [((16, 8, 3, 3), 1, 2, 8, 4), ((12, 6, 3, 3), 2, 2, 8, 4), ((40, 24), 1, 6, 8, 4),
                                              ((8, 3, 3, 3), 1, 1, 8, 8)])
def test_sweeps_never_raise_the_objective(shape, grp, M, K, Cs):
    w, G, ctrd, asmt, _ = problem(3, shape, grp, M, K, Cs)
    c1, a1, obj, chg = eo.quantize_layer_ec(w, ctrd, asmt, G, grp=grp, sweeps=5, ridge=1e-6)
    assert (np.diff(obj) <= 1e-12 * obj[0]).all() and obj[-1] < obj[0] and chg[0] > 0
    assert abs(obj[-1] - eo.objective(w, c1, a1, G, grp)) <= 1e-12 * obj[-1]
    cin = shape[1]
    assert not c1[M - 1, :, cin - (M - 1) * Cs:].any()


def test_every_step_lowers_the_objective_by_what_it_prices():
    w, G, ctrd, asmt, _ = problem(4, (16, 8, 3, 3), 1, 2, 8, 4)
    st = eo.State(w, ctrd, asmt, G, 1, 0.0)
    j0 = st.objective()
    dl = eo.deltas(st, 1, 4)
    gain = np.minimum(dl.min(axis=1), 0.0).sum()
    eo.assign_step(st, 1, 4)
    j1 = st.objective()
    assert abs((j1 - j0) - gain) <= 1e-10 * j0
    e, hm = st.E.copy(), st.Hm.copy()
    st.refresh()
    assert np.allclose(e, st.E, atol=1e-12) and np.allclose(hm, st.Hm, rtol=1e-10, atol=1e-9)
    eo.update_step(st, 1)
    assert st.objective() <= j1
    e, hm = st.E.copy(), st.Hm.copy()
    st.refresh()
    assert np.allclose(e, st.E, atol=1e-6) and np.allclose(hm, st.Hm, rtol=1e-6, atol=1e-5)


def test_one_shot_update_equals_the_sequential_one_for_1x1():
    w, G, ctrd, asmt, _ = problem(5, (40, 24), 1, 6, 8, 4)
    a, b = eo.State(w, ctrd, asmt, G, 1, 1e-6), eo.State(w, ctrd, asmt, G, 1, 1e-6)
    for m in range(6):
        eo.update_step(a, m, one_shot=True)
        eo.update_step(b, m, one_shot=False)
    assert a.C.tobytes() == b.C.tobytes() and np.allclose(a.Hm, b.Hm, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape,grp,M,K,Cs", [((40, 24), 1, 6, 8, 4), ((24, 10), 2, 3, 8, 4)])
def test_the_1x1_sweep_without_a_resident_hm_equals_the_step_by_step_sweep(shape, grp, M, K, Cs):
    rng = np.random.default_rng(6)
    w = rng.standard_normal(shape).astype(np.float32)
    x = np.maximum(rng.standard_normal((30, 1, 1, shape[1] * grp)) + 0.3, 0).astype(np.float32)
    G = eo.gram(x, grp, 1, 1, 1, 0)[0]
    ctrd, asmt, _ = pq_oracle.quantize_layer(w, M, K, Cs, max_iter=20)
    a, b = eo.State(w, ctrd, asmt, G, grp, 1e-6), eo.State(w, ctrd, asmt, G, grp, 1e-6, lazy=True)
    for _ in range(3):
        a.refresh()
        ra, rb = eo.sweep(a), eo.sweep_1x1(b)
        assert ra == rb and np.array_equal(a.A, b.A) and np.allclose(a.C, b.C, rtol=1e-6, atol=0)
        assert abs(a.objective() - b.objective()) <= 1e-9 * a.objective()
    c1, a1, obj, chg = eo.quantize_layer_ec(w, ctrd, asmt, G, grp=grp, sweeps=3, ridge=1e-6)
    assert np.array_equal(a1.reshape(a.A.shape), a.A) and abs(obj[-1] - a.objective()) <= 1e-9 * obj[-1]


def test_gram_run_length_of_the_python_layer_is_the_kernels():
    """The gram test derives its bound from engine.EC_GRAM_RUN: it must be the run length k_ec_gram is compiled with."""
    import os
    import re
    from conftest import ROOT, pkg
    txt = open(os.path.join(ROOT, "quantized-cnn_amd", "csrc", "qcnn_kernels.h")).read()
    assert int(re.search(r"#define\s+QCNN_EC_GRAM_RUN\s+(\d+)", txt).group(1)) == pkg("engine").EC_GRAM_RUN


def test_gpu_case_table_is_importable_and_obeys_the_shape_rules():
    import test_gpu_quantize_ec as gpu_tests                          # importing needs no GPU: its fixtures create the engine
    assert len(gpu_tests.GRAM_CASES) >= 6 and len(gpu_tests.EC_CASES) >= 4 and gpu_tests.case_shapes_ok()
    for _, n, H, W, C, grp, k, stride, pad in gpu_tests.GRAM_CASES:
        assert C % grp == 0 and H + 2 * pad >= k and W + 2 * pad >= k and stride >= 1 and 8 <= n <= 16
