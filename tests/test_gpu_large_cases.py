"""Feature maps beyond 2^31 and beyond 2^32 bytes per panel through every kernel that addresses them (the lg_* shapes of
tests/table_probe.py).  tests/test_large_cases_cpu.py does the offset arithmetic in exact integers, pins the planner's and the
launchers' choice per shape (table_probe.LARGE_REACH), holds the float64 reference used here to dense_expected and shows that a
source offset wrapped modulo 2^32, or sign-extended at 2^31, leaves the bound used here in exactly the rows it names.

Every case runs THREE images: a panel row is 128 lanes whatever the batch, so the byte offsets inside a panel are the large ones
while a host array stays near 100 MB.  One engine is alive at a time.  Device memory, per engine (every map of the model is
allocated for one panel): lg_in_* 4.43 GB input + 1.11 GB conv map + 1.11 GB ReLU map = 6.7 GB; lg_out 0.07 + 4.43 + 4.43 = 8.9 GB;
lg_dec_* 2.15 + 0.72 + 0.72 = 3.6 GB; the glue table with every map kept 4.43 + 4.43 + 1.09 = 10 GB, fused 5.5 GB; beside about
0.2 GB of staging.  An allocation that fails is a test FAILURE naming the need, never a skip.

  * lg_in_lo (source offsets all through [2^31, 2^32)): every live family — exact builder, MFMA tile, 16-wave sliding and
    symmetric, eight-wave tile and sliding, half-panel tile and sliding — forced through the suite's family descriptors, its own
    code required after the launch, per output ELEMENT against table_probe.dense_expected_by_taps:
    |y - want64| <= gamma(knl^2 M + CsEff + 1) mag.  The exact builder returns the oracle's
    bits on output rows 0 .. 2 and 125 .. 126, the map's last (the oracle runs on two crops of the input: rows 0 .. 3, whose output
    rows 0 .. 2 see the real top padding, and rows 124 .. 126, whose output rows 1 .. 2 are rows 125 .. 126 of the map with the real
    bottom padding).  The LIKE_TILE families return the tile kernel's bits over the whole map.
  * lg_in_hi (source rows 128 .. 131 beyond 2^32) and lg_in_hi_g2 (two groups) do NOT go through the table families here: those
    kernels form the source pixel's byte offset in 32 bits (pixel_off, qcnn_dev.h), which wraps on these two shapes and builds
    output rows 127 .. 131 from source rows 0 .. 3 (tests/test_large_cases_cpu.py; LABBOOK.md, "Large maps", says why the 64-bit
    form is not in the library and how to put it back).  The kernels that do not form that offset run all three input shapes: the
    few-image kernel in forwards of 1 and 3 images (code -11), k_dense on lg_in_hi declared dense within gamma(Cin knl^2 + 1) mag.
  * lg_out (an output panel of 4.43 GB behind a small input): the live families' stores, the ReLU map bit-equal to the conv map's
    clamp, the forward's conv map equal to run_layer's (which also sends unpack beyond 2^32).  The planner cuts no tile of a map
    this large, so no split form and no k_conv_sum launch exists here (asserted on the CPU tier).
  * lg_dec_lo / lg_dec_hi (either side of the decoded panel form's 2^31-byte guard) under the decoded options: code -3 and
    gamma(Cin knl^2 + 1) mag for lo; code -1 (the table kernel), the table bound and the TILE options' bits for hi.
  * The glue kernels on a 132 x 128 x 512 map (4.43 GB): [LRN 5 / 0.75, pool 3 / 2] through forward_host — kept maps: LRN inside
    glue_ref.lrn_bound, pool bit-identical to glue_ref.pool; one stream, nothing kept: the fused kernel ran, returns the separate
    pair's bits and lies inside glue_ref.lrn_pool_interval."""
import functools
import time

import numpy as np
import pytest

import glue_ref as gr
import table_probe as tp
from conftest import pkg
from test_gpu_panel_cases import LIKE_TILE, ORDER
from test_gpu_table_probe import BASE, DEC_PANEL, EXACT, OPT, SMALL, TILE, code_ok
from test_panel_cases_cpu import FAMS
from test_table_probe_cpu import oracle_out

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")
capi = pkg("capi")
QcnnError = pkg("engine").QcnnError

N = tp.LARGE_BATCH
IN_SHAPES = ("lg_in_lo", "lg_in_hi", "lg_in_hi_g2")
ORACLE_BOTTOM = 125                       # the exact builder is held to the oracle's bits on output rows 0 .. 2 and from this row to the last


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def model_for(g):
    """[conv, relu]: no FC layer behind maps this large (lg_out's 8.6 M outputs: the FC table kernels form (m Cs) * 512 bytes in
    32 bits, which holds up to 2^23 - 1 input dims only)."""
    return (g["Cin"], g["H"], g["W"]), [topo.conv(g["pad"], g["knl"], g["Ct"], g["grp"], g["stride"]), topo.relu()]


def need_gb(in_chw, layers):
    sizes = topo.fmap_sizes(in_chw, layers)
    return sum(tp.panel_bytes(h, w, c) for h, w, c in sizes) / 1e9


def device_used_gb():
    import torch
    free, total = torch.cuda.mem_get_info(0)
    return (total - free) / 1e9


def make_engine(in_chw, layers, params, opts, dense=False, extra=None):
    """An engine for three images; an allocation that fails is a failure that names the need."""
    eng = pkg("engine").QcnnEngine(0)
    for k, v in dict(BASE, **opts).items():
        eng.set_option(OPT[k], v)
    for k, v in (extra or {}).items():
        eng.set_option(k, v)
    try:
        (eng.load_dense_model if dense else eng.load_model)(in_chw, layers, params, N)
    except QcnnError as e:
        eng.close()
        pytest.fail("loading the model failed (it needs about %.1f GB of device memory for its maps): %s" % (need_gb(in_chw, layers), e))
    return eng


@functools.lru_cache(maxsize=1)
def case(name):
    """Parameters, the three images and the float64 reference of a shape: computed once, shared by the shape's cases, never written."""
    kind, g, M, K, Cs, _ = tp.LARGE_SHAPES[name]
    in_chw, layers = model_for(g)
    spec = synth.quant_spec(in_chw, layers)
    spec[0] = dict(spec[0], M=M, K=K, Cs=Cs)
    params = synth.make_params(in_chw, layers, seed=211, spec=spec)
    x = tp.activations(kind, g, N, seed=212, scaled=False)
    want64, mag = tp.dense_expected_by_taps(g, x, params[0])
    for a in (x, want64, mag):
        a.setflags(write=False)
    return dict(g=g, M=M, K=K, Cs=Cs, in_chw=in_chw, layers=layers, params=params, x=x, want64=want64, mag=mag,
                n_terms=tp.dense_count(kind, g, M, Cs))


def run_family(name, f, label=None):
    """run_layer under a family's options: (y, engine still open).  The family's own code is required."""
    c = case(name)
    eng = make_engine(c["in_chw"], c["layers"], c["params"], f["opts"])
    used = device_used_gb()
    y = eng.run_layer(0, c["x"], N)
    got = eng.layer_split(0)
    what = "%s / %s" % (name, label or f["label"])
    assert code_ok(f["code"], got), "%s: family code %r, expected %r" % (what, got, f["code"])
    r = tp.dense_check(y, c["want64"], c["mag"], c["n_terms"], what=what)
    print("%s: code %r worst err / bound %.3f, device memory in use %.1f GB" % (what, got, r, used))
    assert r <= 1.0
    return y, eng


_TILE = {}                                # the tile kernel's map of ONE shape: computed once, shared by the shape's cases, never written


def keep_tile(name, y):
    y.setflags(write=False)
    _TILE.clear()
    _TILE[name] = y
    return y


def tile_out(name):
    if name not in _TILE:
        y, eng = run_family(name, TILE)
        eng.close()
        keep_tile(name, y)
    return _TILE[name]


def families(name):
    live = tp.LARGE_REACH[name]["live"]
    return ["exact", "tile"] + [k for k in ORDER if k != "tile" and k in live]


def descriptor(key):
    return EXACT if key == "exact" else TILE if key == "tile" else FAMS[key]


def timed(fn):
    @functools.wraps(fn)
    def wrapper(*a, **kw):
        t0 = time.time()
        try:
            return fn(*a, **kw)
        finally:
            print("%s%r: %.1f s" % (fn.__name__, a + tuple(kw.values()), time.time() - t0))
    return wrapper


# ---------------------------------------------------------------- input maps beyond 2^31 / 2^32 bytes ----
@pytest.mark.parametrize("name, key", [(n, k) for n in IN_SHAPES if n not in tp.LARGE_WRAPPING for k in families(n)])
@timed
def test_input_panel_through_a_table_family(name, key):
    c = case(name)
    g = c["g"]
    f = descriptor(key)
    if key == "tile":
        y = tile_out(name)
    else:
        y, eng = run_family(name, f)
        eng.close()
    if key == "exact":                       # the oracle's bits on the rows the CPU tier names, from two crops of the input
        top = oracle_out("conv", dict(g, H=4), c["params"][0], c["x"][:, :4])
        assert np.array_equal(y[:, 0:3], top[:, 0:3]), "%s: output rows 0 .. 2 differ from the oracle's in %d elements" % (
            name, int((y[:, 0:3] != top[:, 0:3]).sum()))
        lo, hi = ORACLE_BOTTOM, tp.out_hw(g)[0]
        bottom = oracle_out("conv", dict(g, H=g["H"] - (lo - 1)), c["params"][0], c["x"][:, lo - 1:])
        assert bottom.shape[1] == hi - lo + 1
        diff = (y[:, lo:hi] != bottom[:, 1:]).reshape(N, hi - lo, -1).any(-1).any(0)
        assert not diff.any(), "%s: output rows %s differ from the oracle's" % (name, [lo + int(i) for i in np.nonzero(diff)[0]])
    if key in LIKE_TILE:
        t = tile_out(name)
        rows = (y != t).reshape(N, y.shape[1], -1).any(-1).any(0)
        assert not rows.any(), "%s / %s: output rows %s differ from the tile kernel's" % (name, f["label"], [int(i) for i in np.nonzero(rows)[0]])


@pytest.mark.parametrize("name", IN_SHAPES)
@timed
def test_input_panel_through_the_few_image_kernel(name):
    c = case(name)
    inp = np.ascontiguousarray(c["x"].transpose(0, 3, 1, 2))
    eng = make_engine(c["in_chw"], c["layers"], c["params"], SMALL["opts"])
    for n in SMALL["n"]:
        eng.forward_host(inp[:n], want_top5=False)
        got = eng.layer_split(0)
        assert got == SMALL["code"], "%s / few-image / %d images: family code %r" % (name, n, got)
        y = eng.layer_output(1, n)
        r = tp.dense_check(y, c["want64"][:n], c["mag"][:n], c["n_terms"], what="%s / few-image / %d images" % (name, n))
        print("%s / few-image / %d images: code %r worst err / bound %.3f" % (name, n, got, r))
        assert r <= 1.0
        assert same_bits(eng.layer_output(2, n), np.maximum(y, np.float32(0)))
    eng.close()


def dense_by_taps64(g, x, bias, weights):
    """(want64, mag) of the precise path at stride 1: the plain zero-padded convolution, float64, one matrix product per tap."""
    assert g["stride"] == 1 and g["grp"] == 1
    x = np.asarray(x, np.float32)
    n, H, W, Cin = x.shape
    knl, pad = g["knl"], g["pad"]
    Ho, Wo = tp.out_hw(g)
    w = np.ascontiguousarray(np.asarray(weights, np.float32).astype(np.float64).transpose(2, 3, 1, 0))    # [kh, kw, Cin, Ct]
    b = np.asarray(bias, np.float32).astype(np.float64)
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, Cin))
    xp[:, pad:pad + H, pad:pad + W] = x
    want, mag = np.tile(b, (n, Ho, Wo, 1)), np.tile(np.abs(b), (n, Ho, Wo, 1))
    for kh in range(knl):
        for kw in range(knl):
            sl = xp[:, kh:kh + Ho, kw:kw + Wo]
            want += sl @ w[kh, kw]
            mag += np.abs(sl) @ np.abs(w[kh, kw])
    return want, mag


@timed
def test_input_panel_through_the_dense_kernel():
    """k_dense on lg_in_hi declared dense: bias plus Cin knl^2 fused multiply-adds in any order."""
    c = case("lg_in_hi")
    g = c["g"]
    dense = {0: synth.make_dense_params(c["in_chw"], c["layers"], seed=213)[0]}
    want64, mag = dense_by_taps64(g, c["x"], dense[0]["bias"], dense[0]["weights"])
    eng = make_engine(c["in_chw"], c["layers"], dense, {}, dense=True)
    y = eng.run_layer(0, c["x"], N)
    eng.close()
    r = tp.dense_check(y, want64, mag, g["Cin"] * g["knl"] ** 2 + 1, what="lg_in_hi / k_dense")
    print("lg_in_hi / k_dense: worst err / bound %.3f" % r)
    assert r <= 1.0


# ---------------------------------------------------------------- an output map beyond 2^32 bytes ----
@pytest.mark.parametrize("key", families("lg_out"))
@timed
def test_output_panel_through_a_table_family(key):
    c = case("lg_out")
    f = descriptor(key)
    y, eng = run_family("lg_out", f)
    if key == "tile":
        keep_tile("lg_out", y)             # the largest case of the file runs once: the LIKE_TILE cases compare with this map
    inp = np.ascontiguousarray(c["x"].transpose(0, 3, 1, 2))
    eng.forward_host(inp, want_prob=False, want_top5=False)
    got = eng.layer_split(0)
    assert code_ok(f["code"], got), "lg_out / %s, forward: family code %r" % (f["label"], got)
    conv = eng.layer_output(1, N)
    assert same_bits(conv, y), "lg_out / %s: the forward's conv map differs from run_layer's in %d elements" % (f["label"], int((conv != y).sum()))
    relu = eng.layer_output(2, N)
    eng.close()
    assert same_bits(relu, np.maximum(y, np.float32(0))), "lg_out / %s: the ReLU map is not the conv map's clamp" % f["label"]
    if key in LIKE_TILE:
        assert same_bits(y, tile_out("lg_out")), "lg_out / %s: differs from the tile kernel's bits" % f["label"]


# ---------------------------------------------------------------- either side of the decoded form's guard ----
@pytest.mark.parametrize("name, code", [("lg_dec_lo", DEC_PANEL["code"]), ("lg_dec_hi", TILE["code"])])
@timed
def test_decoded_panel_form_either_side_of_its_guard(name, code):
    c = case(name)
    g = c["g"]
    want64, mag = tp.dense_expected_one_subspace(g, c["x"], c["params"][0])
    assert np.array_equal(want64, c["want64"]) or tp.dense_check_rel(c["want64"], want64, mag, 2.0 ** -40) <= 1.0    # the two references agree
    eng = make_engine(c["in_chw"], c["layers"], c["params"], DEC_PANEL["opts"])
    y = eng.run_layer(0, c["x"], N)
    got = eng.layer_split(0)
    eng.close()
    assert got == code, "%s under the decoded options: family code %r, expected %r" % (name, got, code)
    if name == "lg_dec_lo":
        r = tp.dense_check_rel(y, want64, mag, tp.dec_dense_rel("conv", g), what=name + " / decoded, panel form")
    else:
        r = tp.dense_check(y, want64, mag, c["n_terms"], what=name + " / table kernel behind the guard")
        assert same_bits(y, tile_out(name)), "%s: the fall-back differs from the same layer under the tile options" % name
    print("%s: code %r worst err / bound %.3f" % (name, got, r))
    assert r <= 1.0


# ---------------------------------------------------------------- glue kernels on a 4.43 GB map ----
@timed
def test_glue_kernels_on_a_map_beyond_4_gib():
    H, W, C = tp.LARGE_GLUE_MAP
    n, alp, bet, ini = 5, 0.01, 0.75, 1.0
    layers = [topo.lorn(n, alp, bet, ini), topo.pool(0, 3, 2)]
    x = gr.signed_log_uniform((N, H, W, C), seed=214, span=3.0)
    y64, s = gr.lrn64(x, n, alp, bet, ini)
    b = gr.lrn_bound(y64, s, n, bet, False)
    inp = gr.nchw(x)

    def forward(eng):
        prob, _ = eng.forward_host(inp, want_top5=False)
        h, w, c = eng.fm_dims(eng.L)
        return prob.reshape(N, h, w, c)
    sep = make_engine((C, H, W), layers, {}, {}, extra={capi.OPT_KEEP_ALL: 1})
    ys = forward(sep)
    lrn = sep.layer_output(1, N)
    sep.close()
    r_lrn = gr.check_bound(lrn, y64, b, "k_lrn_stream on a %d x %d x %d map" % (H, W, C))
    gr.check_exact(ys, gr.pool(lrn, 3, 2, 0), "k_pool4 on a %d x %d x %d map" % (H, W, C))
    fus = make_engine((C, H, W), layers, {}, {}, extra={capi.OPT_KEEP_ALL: 0, capi.OPT_STREAMS: 1, capi.OPT_HOST_CHUNK: 0})
    yf = forward(fus)
    with pytest.raises(RuntimeError):
        fus.layer_output_range(1, 0, 1)                      # the normalised map of a fused pair does not exist: the fused kernel ran
    fus.close()
    r_fused = gr.check_interval(yf, *gr.lrn_pool_interval(y64, b), "k_lrn_pool on a %d x %d x %d map" % (H, W, C))
    assert same_bits(yf, ys), "fused and separate kernels differ in %d elements" % int((yf != ys).sum())
    print("glue on %d x %d x %d: LRN worst err / bound %.3f, fused worst distance / interval %.3f" % (H, W, C, r_lrn, r_fused))
    assert r_lrn <= 1.0 and r_fused <= 1.0
