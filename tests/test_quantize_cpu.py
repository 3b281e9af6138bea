"""Dense -> Q-CNN quantisation, CPU tier: the dense <-> sub-vector map (quantize.decode_layer) against the C oracle's precise
and approximate paths, the numpy restatement of the k-means contract (tests/pq_oracle.py), the parameter-directory round trip,
and the C-ABI entry point failing cleanly without a GPU."""
import numpy as np
import pytest

import pq_oracle
import pyoracle as po
from conftest import has_gpu, pkg, rel_err

topo = pkg("topology")
synth = pkg("synth")
fileio = pkg("fileio")
capi = pkg("capi")
quantize = pkg("quantize")


def dense_shape(in_chw, layers, i):
    sizes = topo.fmap_sizes(in_chw, layers)
    h, w, c = sizes[i]
    ly = layers[i]
    if ly["type"] == topo.CONV:
        return (ly["cnt"], c // ly["grp"], ly["knl"], ly["knl"])
    return (ly["nod"], h * w * c)


def decoded(in_chw, layers, params):
    return {i: dict(bias=p["bias"], weights=quantize.decode_layer(p["ctrd"], p["asmt"], dense_shape(in_chw, layers, i)))
            for i, p in params.items()}


@pytest.mark.parametrize("model", ["tiny", "AlexNet"])
def test_decode_layer_matches_the_approximate_path(model):
    """The precise path on decode_layer(P) computes what the approximate path computes on P, layer by layer on the same
    input: pins the map on grouped conv, CsEff < Cs and the FC flatten order.  The precise path's im2col leaves some taps
    out of output row / column 0 of strided layers (src/CaffeEva.cc:1219-1226, reproduced by the oracle): those two
    border lines are not compared there."""
    if model == "tiny":
        in_chw, layers = topo.tiny_model()
        n_img = 3
    else:
        in_chw, layers, _, _ = topo.MODELS[model]
        n_img = 1
    params = synth.make_params(in_chw, layers, seed=21)
    imgs = synth.make_images(n_img, in_chw, seed=22)
    aprx = po.COracle(in_chw, layers)
    aprx.set_params(params)
    aprx.forward(imgs)
    prec = po.COracle(in_chw, layers)
    prec.set_dense(decoded(in_chw, layers, params))
    for l in sorted(params):
        x = aprx.fm(l)
        ya, yp = aprx.run_layer(l, x, n_img), prec.run_layer(l, x, n_img)
        if layers[l]["type"] == topo.CONV and layers[l]["stride"] > 1:
            ya, yp = ya[:, 1:, 1:], yp[:, 1:, 1:]
        e_inf, _ = rel_err(yp, ya)
        assert e_inf <= 1e-4, "layer %d: %g" % (l, e_inf)


def test_decode_layer_layout_by_hand():
    ctrd = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)          # M = 2, K = 3, Cs = 4
    asmt = np.array([[[[2, 1]]]], np.uint8)                                   # Ct = 1, kh = kw = 1
    w = quantize.decode_layer(ctrd, asmt, (1, 6, 1, 1))
    assert w.reshape(-1).tolist() == [8, 9, 10, 11, 16, 17]                   # sub-space 1 keeps CsEff = 2 dims
    w2 = quantize.decode_layer(ctrd, asmt.reshape(1, 2), (1, 6))
    assert np.array_equal(w2.reshape(-1), w.reshape(-1))


def _same_up_to_permutation(ctrd, asmt, P, wshape):
    """Same dense weights, and per sub-space the code words in use are a permutation of the ones P uses (dims below
    CsEff); where P uses all K, the whole book is a permutation of P's."""
    assert np.array_equal(quantize.decode_layer(ctrd, asmt, wshape), quantize.decode_layer(P["ctrd"], P["asmt"], wshape))
    M, K, cs = ctrd.shape
    cin = wshape[1]
    a, pa = asmt.reshape(-1, M), P["asmt"].reshape(-1, M)
    for m in range(M):
        cse = min(cin - m * cs, cs)
        used, pused = np.unique(a[:, m]), np.unique(pa[:, m])
        assert len(used) == len(pused), "sub-space %d" % m
        got = {tuple(r) for r in ctrd[m, used, :cse].tolist()}
        assert got == {tuple(r) for r in P["ctrd"][m, pused, :cse].tolist()}, "sub-space %d" % m
        if len(pused) == K:
            assert sorted(map(tuple, ctrd[m, :, :cse].tolist())) == sorted(map(tuple, P["ctrd"][m, :, :cse].tolist()))


@pytest.mark.parametrize("model,layer_ids", [("tiny", None), ("AlexNet", (0, 4, 21))])
def test_oracle_recovers_a_quantised_set_exactly(model, layer_ids):
    if model == "tiny":
        in_chw, layers = topo.tiny_model()
    else:
        in_chw, layers, _, _ = topo.MODELS[model]
    spec = synth.quant_spec(in_chw, layers)
    params = synth.make_params(in_chw, layers, seed=31)
    for i in (layer_ids or sorted(params)):
        P, s = params[i], spec[i]
        wshape = dense_shape(in_chw, layers, i)
        w = quantize.decode_layer(P["ctrd"], P["asmt"], wshape)
        ctrd, asmt, st = pq_oracle.quantize_layer(w, s["M"], s["K"], s["Cs"], max_iter=5)
        assert st["iters"] == 1 and st["sse"] == 0.0 and st["unconverged"] == 0, (i, st)
        _same_up_to_permutation(ctrd, asmt, P, wshape)
        assert asmt.shape == P["asmt"].shape


def test_oracle_contract_details():
    """Seeding order, ties, empty code words and the partial last sub-space on a hand-sized case."""
    rng = np.random.default_rng(5)
    w = rng.standard_normal((7, 20, 2, 1)).astype(np.float32)                 # Cin = 20, Cs = 8: CsEff of sub-space 2 is 4
    ctrd, asmt, st = pq_oracle.quantize_layer(w, 3, 4, 8, max_iter=50)
    assert ctrd.shape == (3, 4, 8) and asmt.shape == (7, 2, 1, 3)
    assert (ctrd[2, :, 4:] == 0).all()
    assert st["sse"] <= st["sse_init"] and st["unconverged"] == 0
    P = pq_oracle.points(w, 3, 8)
    assert np.array_equal(P[2, 0, :4], w[0, 16:20, 0, 0]) and np.array_equal(P[1, 1], w[0, 8:16, 1, 0])
    # every assignment is the nearest code word of the returned book (strict <, lowest k)
    for m in range(3):
        cse = min(20 - 8 * m, 8)
        a, _ = pq_oracle.assign(P[m][None], ctrd[m][None], cse)
        assert np.array_equal(a[0].astype(np.uint8), asmt.reshape(-1, 3)[:, m])
    # max_iter = 0 against a given book: plain encoding, nothing else moves
    ctrd0, asmt0, st0 = pq_oracle.quantize_layer(w, 3, 4, 8, ctrd_init=ctrd, max_iter=0)
    assert np.array_equal(ctrd0, ctrd) and np.array_equal(asmt0, asmt) and st0["iters"] == 0 and st0["sse"] == st["sse"]
    # seeding: K larger than the distinct points repeats point 0 (every remaining distance is 0: lowest n)
    c = pq_oracle.seed(np.array([[1.0], [1.0], [3.0]], np.float32), 4, 1)
    assert c[:, 0].tolist() == [1.0, 3.0, 1.0, 1.0]


def test_quantize_param_dir_round_trip(tmp_path):
    in_chw, layers = topo.tiny_model()
    dense = synth.make_dense_params(in_chw, layers, seed=41)
    synth.write_dense_param_dir(str(tmp_path / "dense"), "tiny", dense)
    stats = quantize.quantize_param_dir(str(tmp_path / "dense"), "tiny", str(tmp_path / "q"), "tinyq", (in_chw, layers),
                                        eng=pq_oracle.OracleEngine(), max_iter=4)
    want, _ = quantize.quantize_model(pq_oracle.OracleEngine(), in_chw, layers, dense, max_iter=4)
    got = synth.load_param_dir(str(tmp_path / "q"), "tinyq", layers)
    assert sorted(got) == sorted(want) == sorted(stats)
    for i in want:
        assert np.array_equal(got[i]["bias"], want[i]["bias"])
        assert np.array_equal(got[i]["ctrd"], want[i]["ctrd"])
        assert np.array_equal(got[i]["asmt"], want[i]["asmt"])
        assert got[i]["bits"] == fileio.min_bits(want[i]["asmt"]) == want[i]["bits"]
        assert 0.0 < stats[i]["rel_err"] < 1.0 and stats[i]["sse"] <= stats[i]["sse_init"]


def test_quantize_symbol_exported_and_fails_cleanly():
    lib = capi.load()
    assert "qcnn_quantize_layer" in capi.declared_symbols()
    w = np.zeros(4 * 8, np.float32)
    ctrd = np.zeros(16, np.float32)
    asmt = np.zeros(4, np.uint8)
    rc = lib.qcnn_quantize_layer(None, 4, 8, 1, 1, 1, 2, 8, w.ctypes.data, None, 3, ctrd.ctypes.data, asmt.ctypes.data, None, None)
    assert rc != 0 and "ctx" in lib.qcnn_last_error(None).decode()


@pytest.mark.skipif(has_gpu(), reason="only meaningful without a GPU")
def test_quantize_has_no_cpu_path(tmp_path):
    engine = pkg("engine")
    with pytest.raises(engine.QcnnError):
        engine.QcnnEngine(0)
    in_chw, layers = topo.tiny_model()
    synth.write_dense_param_dir(str(tmp_path), "tiny", synth.make_dense_params(in_chw, layers, seed=1))
    with pytest.raises(engine.QcnnError):                   # the default engine: no GPU, no quantisation
        quantize.quantize_param_dir(str(tmp_path), "tiny", str(tmp_path / "q"), "q", (in_chw, layers))
