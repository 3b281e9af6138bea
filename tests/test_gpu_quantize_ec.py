"""Error-corrected quantisation on the GPU (qcnn_calib_gram / qcnn_quantize_layer_ec through QcnnEngine and quantize.py)
against the numpy fp64 restatement of the contract (tests/ec_oracle.py).  Trajectories are not compared — a near-tie decided
differently sends two correct runs apart; steps and invariants are.  Every bound is derived where it is used and printed
beside the measured figure."""
import numpy as np
import pytest
import torch

import ec_oracle as eo
import pyoracle as po
from conftest import pkg, rel_err

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")
capi = pkg("capi")
engine = pkg("engine")
quantize = pkg("quantize")
ALEX_IN, ALEX = topo.MODELS["AlexNet"][:2]
U32, U64 = 2.0 ** -24, 2.0 ** -53

# name, n, H, W, C, grp, kh = kw, stride, pad
GRAM_CASES = [
    ("alex_conv1", 8, 227, 227, 3, 1, 11, 4, 0),
    ("alex_conv2", 8, 27, 27, 96, 2, 5, 1, 2),
    ("alex_conv3", 8, 13, 13, 256, 1, 3, 1, 1),
    ("alex_fc7", 16, 1, 1, 4096, 1, 1, 1, 0),
    ("conv_1x1", 8, 9, 9, 24, 1, 1, 1, 0),
    ("stride2_pad1_odd", 8, 11, 11, 16, 1, 3, 2, 1),
]

# name, weight shape, grp, M, K, Cs, input (n, H, W), stride, pad        (Cin per group = shape[1])
EC_CASES = [
    ("fc", (48, 40), 1, 10, 16, 4, (64, 1, 1), 1, 0),
    ("conv3x3", (32, 16, 3, 3), 1, 2, 32, 8, (4, 8, 8), 1, 1),
    ("grouped_partial", (24, 6, 3, 3), 2, 2, 16, 4, (4, 7, 7), 2, 1),          # CsEff of the last sub-space = 2
    ("rgb_like", (16, 3, 5, 5), 1, 1, 32, 8, (4, 12, 12), 2, 0),               # CsEff = 3
]


def case_shapes_ok():
    for _, shape, grp, M, K, Cs, _, _, _ in EC_CASES:
        assert shape[0] % grp == 0 and 2 <= K <= 256 and 1 <= Cs <= 16 and (M - 1) * Cs < shape[1] <= M * Cs
    return True


def post_relu(rng, shape):
    return np.maximum(rng.standard_normal(shape) + 0.3, 0.0).astype(np.float32)


def geom(grp, k, stride, pad):
    return dict(grp=grp, kh=k, kw=k, stride=stride, pad=pad)


def gamma(r, u=U32):
    return r * u / (1.0 - r * u)


@pytest.fixture(scope="module")
def eng():
    e = engine.QcnnEngine(0)
    yield e
    e.close()


def ec_problem(eng, case, seed):
    _, shape, grp, M, K, Cs, (n, H, W), stride, pad = case
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(shape).astype(np.float32)
    k = shape[2] if len(shape) == 4 else 1
    x = post_relu(rng, (n, H, W, shape[1] * grp))
    G, _ = eo.gram(x, grp, k, k, stride, pad)
    ctrd, asmt, st = eng.quantize_layer(w, M, K, Cs, max_iter=20)
    return w, G, ctrd, asmt, grp, (M, K, Cs)


# ---------------------------------------------------------------- 1. gram ----
@pytest.mark.parametrize("case", GRAM_CASES, ids=[c[0] for c in GRAM_CASES])
def test_gram_vs_oracle(eng, case):
    name, n, H, W, C, grp, k, stride, pad = case
    x = post_relu(np.random.default_rng(70), (n, H, W, C))
    want, scale = eo.gram(x, grp, k, k, stride, pad)
    g = geom(grp, k, stride, pad)
    got = eng.calib_gram(x, g)
    # fp32 runs of EC_GRAM_RUN patches on a depth-4 MFMA, fp64 across runs: gamma_r * sum |s_p s_q|, r = run + 4
    bound = gamma(engine.EC_GRAM_RUN + 4) * scale
    err = np.abs(got - want)
    print("%s: worst |G - G64| / bound = %.3g" % (name, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    assert np.array_equal(got, got.transpose(0, 2, 1)), "not symmetric to the bit"
    assert got.tobytes() == eng.calib_gram(x, g).tobytes(), "two runs differ"
    h = n // 2
    two = eng.calib_gram(x[h:], g, eng.calib_gram(x[:h], g))
    assert (np.abs(two - want) <= bound).all() and np.array_equal(two, two.transpose(0, 2, 1))


# ---------------------------------------------------------------- 2. + 3. objective, never worse ----
@pytest.mark.parametrize("case", EC_CASES, ids=[c[0] for c in EC_CASES])
def test_objective_matches_oracle_and_never_rises(eng, case):
    w, G, ctrd, asmt, grp, (M, K, Cs) = ec_problem(eng, case, 71)
    ridge = 1e-6
    c1, a1, st = eng.quantize_layer_ec(w, M, K, Cs, G, ctrd, asmt, grp=grp, sweeps=5, ridge=ridge)
    tr = st["obj_trace"]
    for got, want in ((tr[0], eo.objective(w, ctrd, asmt, G, grp)), (tr[-1], eo.objective(w, c1, a1, G, grp))):
        assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    # The search prices a step with P + Cs^2 + Cs fp64 products; a step whose true gain is below the rounding of that sum may be
    # taken: per sweep at most u64 * terms * sum |e_p G_pq e_q| (the absolute objective).  The ridge never raises J: delta = 0 is
    # feasible for the regularised problem.
    s0 = eo.State(w, ctrd, asmt, G, grp)
    absJ = float(sum(np.einsum("ip,pq,iq->", np.abs(s0.E[s0.grp_of == g]), np.abs(s0.G[g]), np.abs(s0.E[s0.grp_of == g]))
                     for g in range(grp)))
    slack = U64 * (s0.P + Cs * Cs + Cs) * absJ
    rise = float(np.max(np.diff(tr)))
    print("%s: J %s, changed %s, largest rise %.3g (slack %.3g)" % (case[0], tr, st["changed"], rise, slack))
    assert rise <= slack
    assert tr[-1] < tr[0]
    assert st["changed"][0] > 0 and np.isfinite(c1).all()
    cin = case[1][1]
    assert not c1.reshape(M, K, Cs)[M - 1, :, cin - (M - 1) * Cs:].any(), "dims >= CsEff must stay 0"
    again = eng.quantize_layer_ec(w, M, K, Cs, G, ctrd, asmt, grp=grp, sweeps=5, ridge=ridge)
    assert again[0].tobytes() == c1.tobytes() and again[1].tobytes() == a1.tobytes(), "two runs differ"


def test_zero_sweeps_return_the_start(eng):
    w, G, ctrd, asmt, grp, (M, K, Cs) = ec_problem(eng, EC_CASES[0], 72)
    c0, a0, st0 = eng.quantize_layer_ec(w, M, K, Cs, G, ctrd, asmt, grp=grp, sweeps=0)
    assert c0.tobytes() == ctrd.tobytes() and np.array_equal(a0, asmt) and len(st0["obj_trace"]) == 1
    assert abs(st0["obj"] - eo.objective(w, ctrd, asmt, G, grp)) <= 1e-9 * st0["obj"]


# ---------------------------------------------------------------- 4. each step is a near-minimiser ----
def test_single_steps_are_near_minimisers(eng):
    rng = np.random.default_rng(73)
    Ct, D, K = 64, 4, 8
    w = rng.standard_normal((Ct, D)).astype(np.float32)
    x = post_relu(rng, (50, 1, 1, D))
    G = eo.gram(x, 1, 1, 1, 1, 0)[0]
    ctrd, asmt, _ = eng.quantize_layer(w, 1, K, D, max_iter=3)
    ridge = 1e-6
    c1, a1, st = eng.quantize_layer_ec(w, 1, K, D, G, ctrd, asmt, sweeps=1, ridge=ridge)
    # assign: the cost of the returned assignment against the fp64 minimum, both priced with the START book
    s = eo.State(w, ctrd, asmt, G, 1, ridge)
    dl = eo.deltas(s, 0, 0)
    c = ctrd[0].astype(np.float64)
    d = c[None] - c[asmt[:, 0]][:, None]
    mag = 2.0 * np.einsum("ckj,cj->ck", np.abs(d), np.abs(s.Hm)) + np.einsum("cki,ij,ckj->ck", np.abs(d), np.abs(G[0]), np.abs(d))
    tol = U64 * (D * D + 2 * D) * mag.max(axis=1)                  # rounding of the D^2 + 2 D products of one delta, in fp64
    chosen = dl[np.arange(Ct), a1[:, 0]]
    best = np.minimum(dl.min(axis=1), 0.0)
    print("assign: worst (chosen - best) %.3g, tolerance >= %.3g" % (float((chosen - best).max()), float(tol.min())))
    assert (chosen <= best + tol).all()
    # update: the returned code words against the normal equations at the state the assign step left behind
    for ct in range(Ct):
        s.A[ct, 0, 0] = a1[ct, 0]
    s.refresh()
    worst = 0.0
    for k in range(K):
        if not (a1[:, 0] == k).any():
            assert c1[0, k].tobytes() == ctrd[0, k].tobytes()
            continue
        A, v = eo.normal_equations(s, 0, k)
        A = A + s.lam * np.eye(D)
        delta = c1[0, k].astype(np.float64) - c[k]
        res = np.abs(A @ delta - v)
        # c_k is stored in fp32: it may sit u32 |c_k| off the exact solution; the sums of A delta and v round in fp64
        nk = int((a1[:, 0] == k).sum())
        bound = np.abs(A) @ (U32 * np.abs(c1[0, k].astype(np.float64))) + U64 * (nk + D) * (np.abs(A) @ np.abs(delta) + np.abs(s.Hm[a1[:, 0] == k]).sum(axis=0))
        worst = max(worst, float((res / bound).max()))
        assert (res <= bound).all(), (k, res, bound)
    print("update: worst residual / bound = %.3g" % worst)


# ---------------------------------------------------------------- 5. reduces to k-means ----
def test_identity_gram_at_a_kmeans_fixed_point_changes_nothing(eng):
    rng = np.random.default_rng(74)
    M, K, Cs, shape = 4, 16, 4, (96, 16, 3, 3)
    book = (rng.standard_normal((M, K, Cs)) * 2.0).astype(np.float32)
    a = rng.integers(0, K, size=(shape[0], 3, 3, M), dtype=np.uint8)
    w = quantize.decode_layer(book, a, shape) + (rng.standard_normal(shape) * 1e-3).astype(np.float32)
    ctrd, asmt, st = eng.quantize_layer(w, M, K, Cs, ctrd_init=book, max_iter=50)
    assert st["unconverged"] == 0 and np.array_equal(asmt, a)
    ridge = 1e-6
    c1, a1, ec = eng.quantize_layer_ec(w, M, K, Cs, None, ctrd, asmt, sweeps=3, ridge=ridge)
    assert not ec["changed"].any() and np.array_equal(a1, asmt)
    if c1.tobytes() == ctrd.tobytes():                              # a sweep that changed nothing ends the search: the trace repeats
        assert ec["obj_trace"][1] == ec["obj_trace"][2] == ec["obj_trace"][3]
    # G = I: A_k = (n_k + lambda) I, v_k = n_k (mean_k - c_k), and c_k is the mean rounded to fp32: |v_k| <= n_k u32 |c_k|, so
    # |delta| <= u32 |c_k|, shrunk (not grown) by lambda = ridge; stored in fp32 the word moves by at most one more rounding
    bound = 2.0 * U32 * np.abs(ctrd.astype(np.float64)) * (1.0 + ridge) + 1e-45
    move = np.abs(c1.astype(np.float64) - ctrd.astype(np.float64))
    print("largest move / bound = %.3g" % float((move / bound).max()))
    assert (move <= bound).all()
    assert abs(ec["obj_init"] - st["sse"]) <= 1e-6 * st["sse"]            # J with G = I is the k-means SSE (fp32 distances there)


# ---------------------------------------------------------------- 6. it does what it is for ----
def held_out_errors(in_chw, layers, dense, P_list, ids, held):
    """Response error of layers `ids` through the engine: run_layer of each quantised set against run_layer of the dense layer."""
    n = len(held)
    ed = engine.QcnnEngine(0)
    ed.load_dense_model(in_chw, layers, dense, n)
    ed.forward_host(held, want_prob=False, want_top5=False)
    X = {i: quantize.layer_input(layers, i, ed.layer_output(i, n)) for i in ids}
    ref = {i: ed.run_layer(i, X[i], n).astype(np.float64) for i in ids}
    ed.close()
    errs = []
    for P in P_list:
        e = engine.QcnnEngine(0)
        e.load_model(in_chw, layers, P, n)
        errs.append({i: float(((e.run_layer(i, X[i], n).astype(np.float64) - ref[i]) ** 2).sum()) for i in ids})
        e.close()
    return errs, X, ref


def numpy_response(w_patch, Xp, grp):
    """[rows][Ct] float64 responses (no bias) of weights in patch order [Ct][P] on patches [grp][rows][P]."""
    ctg = w_patch.shape[0] // grp
    return np.concatenate([Xp[g] @ w_patch[g * ctg:(g + 1) * ctg].T for g in range(grp)], axis=1)


def oracle_ratio(w, km, G, Xp, ref, grp, sweeps, ridge):
    """The oracle's held-out figure, measured as the engine's is: squared distance of the quantised layer's response to the
    reference response ``ref`` [rows][Ct] (bias removed) after error correction over that of the k-means start."""
    print("  oracle: %d sweep(s) on weights %r ..." % (sweeps, w.shape), flush=True)
    c, a, _, _ = eo.quantize_layer_ec(w, km[0], km[1], G, grp=grp, sweeps=sweeps, ridge=ridge)
    cin, taps = eo.dims(w)[1], eo.dims(w)[2] * eo.dims(w)[3]
    err = lambda cc, aa: float(((numpy_response(eo.decode(cc, aa, cin, taps), Xp, grp) - ref) ** 2).sum())
    return err(c, a) / err(km[0], km[1])


def check_it_helps(eng, in_chw, layers, ids, n_cal, sweeps, seed):
    dense = synth.make_dense_params(in_chw, layers, seed=seed)
    cal = synth.make_images(n_cal, in_chw, seed=seed + 1)
    held = synth.make_images(n_cal, in_chw, seed=seed + 2)
    ec_eng = engine.QcnnEngine(0)
    calib = quantize.calibrate(ec_eng, in_chw, layers, dense, cal)
    ec_eng.close()
    calib = {i: calib[i] for i in ids}
    ridge = engine.DEFAULT_EC_RIDGE
    P_km, _ = quantize.quantize_model(eng, in_chw, layers, dense, max_iter=10)
    P_ec, stats = quantize.quantize_model(eng, in_chw, layers, dense, max_iter=10, calib=calib, sweeps=sweeps, ridge=ridge)
    (e_km, e_ec), X, ref = held_out_errors(in_chw, layers, dense, [P_km, P_ec], ids, held)
    spec = synth.quant_spec(in_chw, layers)
    for i in ids:
        ratio = e_ec[i] / e_km[i]
        g = quantize.layer_geom(layers, i)
        Xp = eo.patches(X[i], g["grp"], g["kh"], g["kw"], g["stride"], g["pad"])
        w = dense[i]["weights"]
        # seed 0 against the ENGINE's dense response (the precise path reproduces the reference's im2col, which leaves a few
        # taps out at output row / column 0 of strided layers: both figures must carry that same constant term)
        ref0 = ref[i].reshape(-1, w.shape[0]) - dense[i]["bias"].astype(np.float64)[None, :]
        ors = [oracle_ratio(w, (P_km[i]["ctrd"], P_km[i]["asmt"]), calib[i], Xp, ref0, g["grp"], sweeps, ridge)]
        s = spec[i]
        for sd in (1, 2):                                         # the oracle's own spread over the seed of the weights
            w2 = (np.random.default_rng(seed + 10 * sd + i).standard_normal(w.shape) * w.std()).astype(np.float32)
            c2, a2, _ = eng.quantize_layer(w2, s["M"], s["K"], s["Cs"], max_iter=10)
            ors.append(oracle_ratio(w2, (c2, a2), calib[i], Xp, numpy_response(eo.to_patch_order(w2), Xp, g["grp"]), g["grp"], sweeps, ridge))
        margin = max(ors) - min(ors)
        print("layer %d: held-out response error after / before error correction: engine %.4f, oracle %.4f (seeds %s, margin %.4f); "
              "calibration J %.4g -> %.4g" % (i, ratio, ors[0], ["%.4f" % r for r in ors], margin, stats[i]["obj_init"], stats[i]["obj"]))
        assert ratio < 1.0, (i, ratio)
        assert abs(ratio - ors[0]) <= margin, (i, ratio, ors)


def test_error_correction_lowers_held_out_response_error_tiny(eng):
    in_chw, layers = topo.tiny_model()
    ids = [i for i, ly in enumerate(layers) if ly["type"] in (topo.CONV, topo.FCNT)]
    check_it_helps(eng, in_chw, layers, ids, 48, engine.DEFAULT_EC_SWEEPS, 75)


def test_error_correction_lowers_held_out_response_error_alexnet_conv3_fc7(eng):
    check_it_helps(eng, ALEX_IN, ALEX, [8, 18], 32, 1, 76)


# ---------------------------------------------------------------- 7. flow, isolation, bad arguments ----
def test_flow_through_engine_and_oracle(eng):
    in_chw, layers = topo.tiny_model()
    dense = synth.make_dense_params(in_chw, layers, seed=77)
    imgs = synth.make_images(40, in_chw, seed=78)
    ce = engine.QcnnEngine(0)
    calib = quantize.calibrate(ce, in_chw, layers, dense, imgs[:32], chunk=12)
    ce.close()
    params, stats = quantize.quantize_model(eng, in_chw, layers, dense, calib=calib)
    plain, _ = quantize.quantize_model(eng, in_chw, layers, dense)
    spec = synth.quant_spec(in_chw, layers)
    for i, p in plain.items():
        c, a, _ = eng.quantize_layer(dense[i]["weights"], spec[i]["M"], spec[i]["K"], spec[i]["Cs"])
        assert c.tobytes() == p["ctrd"].tobytes() and a.tobytes() == p["asmt"].tobytes()
        assert stats[i]["obj"] < stats[i]["obj_init"] and len(stats[i]["changed"]) == engine.DEFAULT_EC_SWEEPS
    e = engine.QcnnEngine(0)
    e.load_model(in_chw, layers, params, 40)
    prob, _ = e.forward_host(imgs)
    e.close()
    orc = po.COracle(in_chw, layers)
    orc.set_params(params)
    orc.forward(imgs[:8])
    e_inf, e_l2 = rel_err(prob[:8], orc.fm(len(layers)).reshape(8, -1))
    assert e_inf <= 1e-4 and e_l2 <= 1e-4, (e_inf, e_l2)


def test_ec_leaves_a_loaded_model_alone():
    in_chw, layers = topo.tiny_model()
    params = synth.make_params(in_chw, layers, seed=79)
    imgs = synth.make_images(9, in_chw, seed=80)
    rng = np.random.default_rng(81)
    w = rng.standard_normal((256, 512)).astype(np.float32)
    x = post_relu(rng, (64, 1, 1, 512))
    e = engine.QcnnEngine(0)
    e.load_model(in_chw, layers, params, 9)
    before = e.forward_host(imgs)
    ctrd, asmt, _ = e.quantize_layer(w, 128, 32, 4, max_iter=2)
    e.sync()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        G = e.calib_gram(x, geom(1, 1, 1, 0))
        e.quantize_layer_ec(w, 128, 32, 4, G, ctrd, asmt, sweeps=1)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    after = e.forward_host(imgs)
    e.close()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert abs(free1 - free0) <= (1 << 20), (free0, free1)


def test_bad_arguments_are_refused(eng):
    w, G, ctrd, asmt, grp, (M, K, Cs) = ec_problem(eng, EC_CASES[1], 82)
    ok = dict(M=M, K=K, Cs=Cs, gram=G, ctrd=ctrd, asmt=asmt, grp=1, sweeps=2, ridge=1e-6)
    lib = capi.load()
    ct, cin, kh, kw = w.shape

    def call(**kw_):
        a = dict(ok)
        a.update(kw_)
        c1, a1 = np.empty((a["M"], a["K"], a["Cs"]), np.float32), np.empty(asmt.shape, np.uint8)
        ptr = lambda v: v.ctypes.data if v is not None else None
        return lib.qcnn_quantize_layer_ec(eng.h, ct, cin, a["grp"], kh, kw, a["M"], a["K"], a["Cs"], a.get("w", w).ctypes.data, ptr(a["gram"]),
                                          ptr(a["ctrd"]), ptr(a["asmt"]), a["sweeps"], a["ridge"], c1.ctypes.data, a1.ctypes.data, None, None)

    bad_a = asmt.copy(); bad_a.flat[5] = K
    wn = w.copy(); wn[1, 2, 0, 1] = np.inf
    gn = G.copy(); gn[0, 3, 4] = np.nan
    gd = G.copy(); gd[0, 7, 7] = -1.0
    cn = ctrd.copy(); cn[0, 1, 2] = np.nan
    for kw_ in (dict(K=1), dict(K=257), dict(Cs=0), dict(Cs=17), dict(M=1), dict(M=4), dict(grp=5), dict(grp=0), dict(sweeps=-1),
                dict(ridge=-1e-3), dict(w=wn), dict(gram=gn), dict(gram=gd), dict(ctrd=cn), dict(asmt=bad_a), dict(ctrd=None), dict(asmt=None)):
        assert call(**kw_) != 0, kw_
        assert lib.qcnn_last_error(eng.h).decode().startswith("qcnn_quantize_layer_ec:"), (kw_, lib.qcnn_last_error(eng.h))
    x = post_relu(np.random.default_rng(83), (2, 6, 6, 8))
    for g in (geom(3, 3, 1, 1), geom(1, 0, 1, 0), geom(1, 3, 0, 0), geom(1, 3, 1, -1), geom(1, 9, 1, 0)):
        with pytest.raises(engine.QcnnError, match="qcnn_calib_gram"):
            eng.calib_gram(x, g)
    assert call() == 0                                              # the context is still usable
    want = eo.gram(x, 1, 3, 3, 1, 1)[0]
    assert np.allclose(eng.calib_gram(x, geom(1, 3, 1, 1)), want, rtol=1e-4, atol=1e-6)
