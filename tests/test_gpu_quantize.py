"""Dense -> Q-CNN quantisation on the GPU (qcnn_quantize_layer through QcnnEngine.quantize_layer and quantize.py):
bit-identical to the numpy restatement of the contract (tests/pq_oracle.py), exact recovery of a quantised set, the flow
through the existing engine / file formats / oracle, isolation from a loaded model, argument checking."""
import ctypes as C

import numpy as np
import pytest
import torch

import pq_oracle
import pyoracle as po
from conftest import pkg, rel_err

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")
fileio = pkg("fileio")
capi = pkg("capi")
engine = pkg("engine")
quantize = pkg("quantize")
TOL = 1e-4
ALEX_IN, ALEX = topo.MODELS["AlexNet"][:2]


def dense_shape(in_chw, layers, i):
    h, w, c = topo.fmap_sizes(in_chw, layers)[i]
    ly = layers[i]
    if ly["type"] == topo.CONV:
        return (ly["cnt"], c // ly["grp"], ly["knl"], ly["knl"])
    return (ly["nod"], h * w * c)


def padded_zero(params, in_chw, layers):
    """P with ctrd zeroed on the dims j >= CsEff, as the shipped files hold them."""
    out = {}
    for i, p in params.items():
        c = p["ctrd"].copy()
        cin = dense_shape(in_chw, layers, i)[1]
        m, _, cs = c.shape
        c[m - 1, :, cin - (m - 1) * cs:] = 0.0
        out[i] = dict(p, ctrd=c)
    return out


@pytest.fixture(scope="module")
def eng():
    e = engine.QcnnEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def alex_p():
    return padded_zero(synth.make_params(ALEX_IN, ALEX, seed=7), ALEX_IN, ALEX)


def check_vs_oracle(eng, w, M, K, Cs, max_iter, ctrd_init=None):
    got = eng.quantize_layer(w, M, K, Cs, ctrd_init=ctrd_init, max_iter=max_iter)
    want = pq_oracle.quantize_layer(w, M, K, Cs, ctrd_init=ctrd_init, max_iter=max_iter)
    assert got[0].tobytes() == want[0].tobytes(), "code book differs"
    assert got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes(), "assignments differ"
    gs, ws = got[2], want[2]
    assert (gs["iters"], gs["unconverged"]) == (ws["iters"], ws["unconverged"]), (gs, ws)
    for key in ("sse_init", "sse"):
        assert abs(gs[key] - ws[key]) <= 1e-9 * max(abs(ws[key]), 1e-30), (key, gs, ws)
    return got


# ---------------------------------------------------------------- 1. bit-identical to the oracle ----
def test_tiny_model_layers_to_convergence(eng):
    in_chw, layers = topo.tiny_model()
    dense = synth.make_dense_params(in_chw, layers, seed=51)
    spec = synth.quant_spec(in_chw, layers)
    for i, d in dense.items():
        s = spec[i]
        _, _, st = check_vs_oracle(eng, d["weights"], s["M"], s["K"], s["Cs"], 200)
        assert st["unconverged"] == 0, (i, st)


@pytest.mark.parametrize("layer", [0, 4, 12, 21])      # conv1 (CsEff = 3), conv2 (grouped), conv5, fc8 (Cs = 1, K = 16)
def test_alexnet_layers_vs_oracle(eng, layer):
    dense = synth.make_dense_params(ALEX_IN, ALEX, seed=52)
    s = synth.quant_spec(ALEX_IN, ALEX)[layer]
    check_vs_oracle(eng, dense[layer]["weights"], s["M"], s["K"], s["Cs"], 8)


@pytest.mark.parametrize("shape,M,K,Cs", [
    ((24, 20, 3, 3), 3, 16, 8),        # partial last sub-space: CsEff = 4
    ((64, 16, 3, 3), 2, 256, 8),       # K = 256
    ((48, 30, 1, 1), 3, 100, 10),      # K = 100, Cs = 10 (not a power of two), partial last
    ((40, 32, 3, 3), 2, 64, 16),       # Cs = 16
    ((300, 64), 16, 32, 4),            # FC
])
def test_other_shapes_vs_oracle(eng, shape, M, K, Cs):
    w = np.random.default_rng(53).standard_normal(shape).astype(np.float32)
    check_vs_oracle(eng, w, M, K, Cs, 25)
    init = np.random.default_rng(54).standard_normal((M, K, Cs)).astype(np.float32)
    check_vs_oracle(eng, w, M, K, Cs, 5, ctrd_init=init)


# ---------------------------------------------------------------- 2. encoding only ----
def test_encoding_against_a_given_book_recovers_the_assignments(eng, alex_p):
    for i, p in alex_p.items():
        M, K, Cs = p["ctrd"].shape
        w = quantize.decode_layer(p["ctrd"], p["asmt"], dense_shape(ALEX_IN, ALEX, i))
        ctrd, asmt, st = eng.quantize_layer(w, M, K, Cs, ctrd_init=p["ctrd"], max_iter=0)
        assert np.array_equal(asmt, p["asmt"]), "layer %d" % i
        assert ctrd.tobytes() == p["ctrd"].tobytes(), "layer %d" % i
        assert st["iters"] == 0 and st["sse"] == 0.0 and st["sse_init"] == 0.0


# ---------------------------------------------------------------- 3. exact recovery end to end ----
def test_exact_recovery_forward_bit_identical(eng, alex_p):
    dense = {i: dict(bias=p["bias"], weights=quantize.decode_layer(p["ctrd"], p["asmt"], dense_shape(ALEX_IN, ALEX, i)))
             for i, p in alex_p.items()}
    params, stats = quantize.quantize_model(eng, ALEX_IN, ALEX, dense)
    assert sorted(params) == sorted(alex_p)
    for i, st in stats.items():
        assert st["iters"] == 1 and st["sse"] == 0.0 and st["unconverged"] == 0 and st["rel_err"] == 0.0, (i, st)
    imgs = synth.make_images(131, ALEX_IN, seed=55)
    for decode in (1, 0):
        outs = []
        for P in (alex_p, params):
            e = engine.QcnnEngine(0)
            e.set_option(capi.OPT_DECODE, decode)
            e.load_model(ALEX_IN, ALEX, P, 131)
            outs.append(e.forward_host(imgs))
            e.close()
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), "decode %d" % decode


# ---------------------------------------------------------------- 4. large layers, self-consistent ----
@pytest.mark.parametrize("layer", [15, 18])             # fc6, fc7
def test_large_fc_layers_self_consistent(eng, layer):
    w = synth.make_dense_params(ALEX_IN, ALEX, seed=56)[layer]["weights"]
    s = synth.quant_spec(ALEX_IN, ALEX)[layer]
    M, K, Cs = s["M"], s["K"], s["Cs"]
    ctrd, asmt, st = eng.quantize_layer(w, M, K, Cs)
    assert st["sse"] <= st["sse_init"] and 1 <= st["iters"] <= engine.DEFAULT_MAX_ITER
    P = pq_oracle.points(w, M, Cs)
    a = asmt.reshape(-1, M)
    sse = 0.0
    step = 128
    for m0 in range(0, M, step):
        am, dm = pq_oracle.assign(P[m0:m0 + step], ctrd[m0:m0 + step], Cs)
        assert np.array_equal(am.astype(np.uint8), a[:, m0:m0 + step].T), "sub-spaces %d.." % m0
        sse += float(dm.astype(np.float64).sum())
    assert abs(sse - st["sse"]) <= 1e-9 * sse
    ctrd2, asmt2, st2 = eng.quantize_layer(w, M, K, Cs)
    assert ctrd2.tobytes() == ctrd.tobytes() and asmt2.tobytes() == asmt.tobytes() and st2 == st
    print("fc layer %d: %s" % (layer, st))


# ---------------------------------------------------------------- 5. flow through the existing library ----
def test_quantized_alexnet_runs_through_engine_files_and_oracle(eng, tmp_path):
    dense = synth.make_dense_params(ALEX_IN, ALEX, seed=57)
    params, stats = quantize.quantize_model(eng, ALEX_IN, ALEX, dense, max_iter=10)
    synth.write_dense_param_dir(str(tmp_path / "dense"), "alex", dense)
    stats_dir = quantize.quantize_param_dir(str(tmp_path / "dense"), "alex", str(tmp_path / "q"), "alexq", "AlexNet", eng=eng,
                                            max_iter=10)
    from_dir = synth.load_param_dir(str(tmp_path / "q"), "alexq", ALEX)
    for i in params:
        assert from_dir[i]["ctrd"].tobytes() == params[i]["ctrd"].tobytes()
        assert np.array_equal(from_dir[i]["asmt"], params[i]["asmt"]) and stats_dir[i]["sse"] == stats[i]["sse"]
    imgs = synth.make_images(131, ALEX_IN, seed=58)
    orc = po.COracle(ALEX_IN, ALEX)
    orc.set_params(params)
    orc.forward(imgs[128:131])
    want = orc.fm(len(ALEX)).reshape(3, -1)
    e = engine.QcnnEngine(0)
    e.load_model(ALEX_IN, ALEX, params, 131)
    prob, top5 = e.forward_host(imgs)
    e.close()
    e = engine.QcnnEngine(0)
    e.load_model(ALEX_IN, ALEX, from_dir, 131, upload=False)
    e.upload_cbn(from_dir)
    prob2, top5b = e.forward_host(imgs)
    e.close()
    assert np.array_equal(prob, prob2) and np.array_equal(top5, top5b)
    e_inf, e_l2 = rel_err(prob[128:131], want)
    assert e_inf <= TOL and e_l2 <= TOL, (e_inf, e_l2)
    # the precise path on the dense weights: recorded, not asserted (synthetic weights carry no trained structure)
    e = engine.QcnnEngine(0)
    e.load_dense_model(ALEX_IN, ALEX, dense, 131)
    prob_d, top5_d = e.forward_host(imgs)
    e.close()
    pe_inf, pe_l2 = rel_err(prob, prob_d)
    print("quantised vs dense AlexNet (synthetic): prob rel err inf %.3g l2 %.3g, top-1 agreement %.3f; per layer %s"
          % (pe_inf, pe_l2, float((top5[:, 0] == top5_d[:, 0]).mean()),
             {i: (round(s["rel_err"], 4), s["iters"]) for i, s in stats.items()}))


# ---------------------------------------------------------------- 6. isolation ----
def test_quantize_leaves_a_loaded_model_alone():
    in_chw, layers = topo.tiny_model()
    params = synth.make_params(in_chw, layers, seed=59)
    imgs = synth.make_images(9, in_chw, seed=60)
    w = synth.make_dense_params(ALEX_IN, ALEX, seed=61)[15]["weights"]       # fc6: the largest scratch
    e = engine.QcnnEngine(0)
    e.load_model(in_chw, layers, params, 9)
    before = e.forward_host(imgs)
    e.sync()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        e.quantize_layer(w, 2304, 32, 4, max_iter=2)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    after = e.forward_host(imgs)
    e.close()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert abs(free1 - free0) <= (1 << 20), (free0, free1)


# ---------------------------------------------------------------- 7. bad arguments ----
def test_bad_arguments_are_refused(eng):
    w = np.random.default_rng(62).standard_normal((8, 16, 3, 3)).astype(np.float32)
    bad = [dict(K=0), dict(K=1), dict(K=257), dict(Cs=0), dict(Cs=17), dict(M=1),   # M*Cs < Cin
           dict(M=3),                                                                  # (M-1)*Cs >= Cin
           dict(max_iter=-1)]
    for kw in bad:
        a = dict(M=2, K=16, Cs=8, max_iter=3)
        a.update(kw)
        with pytest.raises(engine.QcnnError) as ex:
            eng.quantize_layer(w, a["M"], a["K"], a["Cs"], max_iter=a["max_iter"])
        assert "qcnn_quantize_layer" in str(ex.value), kw
    wn = w.copy()
    wn[3, 5, 1, 2] = np.nan
    with pytest.raises(engine.QcnnError, match="not finite"):
        eng.quantize_layer(wn, 2, 16, 8)
    lib = capi.load()
    out_c = np.empty((2, 16, 8), np.float32)
    out_a = np.empty((8, 3, 3, 2), np.uint8)
    for wp, cp, ap in ((None, out_c.ctypes.data, out_a.ctypes.data), (w.ctypes.data, None, out_a.ctypes.data),
                       (w.ctypes.data, out_c.ctypes.data, None)):
        assert lib.qcnn_quantize_layer(eng.h, 8, 16, 3, 3, 2, 16, 8, wp, None, 3, cp, ap, None, None) != 0
        assert "NULL" in lib.qcnn_last_error(eng.h).decode()
    # the context is still usable
    check_vs_oracle(eng, w, 2, 16, 8, 10)
