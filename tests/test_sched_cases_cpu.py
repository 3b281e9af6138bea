"""The exact network of tests/sched_cases.py without a GPU: its integer reference is the oracle's, its data is exact in every
precision a kernel keeps it in, the mistakes a schedule can make are visible on it, and SCHED_REACH is what the planner answers.
Everything is checked on the very batch tests/test_gpu_schedule.py runs (sched_cases.reference(): 1027 images)."""
import numpy as np
import pytest

import f16split_model as fm16
import pyoracle as po
import sched_cases as sc
from test_bf16split_cpu import split3

topo = sc.topo
N = sc.N_MAX
# the largest |bias| + sum |x_j c_j| of any output element per conv / FC layer over the 1027 images, in units (2^0; the last layer
# 2^-18): conv1 45, conv2 4001, conv3 37640, fc1 732404 (2^19.5), fc2 3265215 (2^21.6), fc3 6482648 (2^22.6).  All but the last
# meet the 2^22 aimed for; every one is below 2^24
MAGS = {0: 45, 3: 4001, 5: 37640, 8: 732404, 11: 3265215, 13: 6482648}


@pytest.fixture(scope="module")
def ref():
    x, fm, mags = sc.reference(with_mags=True)
    return dict(x=x, fm=fm, mags=mags, rows=fm[sc.LAST_FC + 1].reshape(N, -1))


def test_reference_is_the_oracle_and_the_plain_look_ups():
    """Images 0, 1 and the last one: the float64-carried reference, the int64 tap-by-tap look-ups and the C oracle agree on every
    conv / FC / ReLU / pool map, bit for bit — the NCHW flatten in front of the first FC layer included."""
    x = sc.inputs()[[0, 1, N - 1]]
    fast = sc.forward_int(np.rint(x.transpose(0, 2, 3, 1)).astype(np.int64))
    plain = sc.reference_plain(x)
    orc = po.COracle(sc.IN_CHW, sc.LAYERS)
    orc.set_params(sc.file_params(sc.params()))
    orc.forward(x)
    assert len(fast) == len(plain) == sc.LAST_FC + 2
    for l in range(sc.LAST_FC + 2):
        assert fast[l].dtype == np.int64 and np.array_equal(fast[l], plain[l]), l
        got = orc.fm(l)
        assert got.shape == fast[l].shape == (3,) + sc.SIZES[l], l
        assert np.array_equal(got, sc.as_float32(fast[l], l)), "fm[%d]" % l
    # the flatten order is part of it: NHWC order gives another fc1 map
    kind, g = sc.geom_of(sc.LAYERS, sc.SIZES, sc.FIRST_FC)
    assert not np.array_equal(sc.fc_int(fast[sc.FIRST_FC].reshape(3, -1), g, sc.params()[sc.FIRST_FC]), fast[sc.FIRST_FC + 1].reshape(3, -1))
    # the LRN table's integer part the same way
    xl = sc.inputs(2, sc.LRN_IN_CHW, sc.SEED + 100)
    sizes = topo.fmap_sizes(sc.LRN_IN_CHW, sc.LRN_LAYERS)
    orl = po.COracle(sc.LRN_IN_CHW, sc.LRN_LAYERS)
    orl.set_params(sc.file_params(sc.lrn_params()))
    orl.forward(xl)
    pl = sc.reference_plain(xl, sc.LRN_LAYERS, sizes, sc.lrn_params(), last=1)
    _, conv, relu = sc.lrn_reference()
    assert np.array_equal(pl[1], conv[:2]) and np.array_equal(pl[2], relu[:2])
    assert np.array_equal(orl.fm(1), conv[:2].astype(np.float32)) and np.array_equal(orl.fm(2), relu[:2].astype(np.float32))


def test_every_partial_sum_is_exact(ref):
    """|bias| + sum |x_j c_j| <= 2^24 units on every output element of every conv / FC layer (MAGS records the largest); parameters are
    integers times one power of two per layer, biases non-zero; the logits stay far inside the un-shifted soft-max's range."""
    print("largest |bias| + sum |x_j c_j| per layer:", {l: (m, "2^%.1f" % np.log2(m)) for l, m in ref["mags"].items()})
    assert ref["mags"] == MAGS
    assert all(m <= sc.F32_UNITS for m in MAGS.values()) and all(MAGS[l] <= 2 ** 22 for l in sc.QLAYERS[:-1])
    for l, p in sc.params().items():
        b, c, _ = sc.int_params(p)
        assert (b != 0).all() and (np.abs(c).sum(-1) % 2 == 1).all(), l           # odd coordinate sums: no entry of a +-1 input is 0
    assert (np.abs(ref["x"]) == 1).all()
    logits = ref["rows"] * sc.unit(sc.LAST_FC + 1)
    assert np.abs(logits).max() <= 16.0, float(np.abs(logits).max())
    assert set(sc.QUANT[l][4] for l in sc.QLAYERS[:-1]) == {0} and sc.QUANT[sc.LAST_FC][4] < 0


def test_first_layer_is_exact_in_one_fp16_and_one_bf16_piece(ref):
    """QCNN_OPT_DEC_BF16SPLIT = 1 / 2: inputs and code words of the layer read in place are exact in ONE bf16 / fp16 piece (64 |x| <= 2048,
    Sw |c| an integer <= 2048 times a power of two), the other pieces are zero, and the models' products give the integer result."""
    p = sc.params()[0]
    x = ref["x"][:5]
    assert (fm16.SX * np.abs(x) <= 2048).all() and not fm16.out_of_range(x).any()
    sw = fm16.layer_scale(p, sc.IN_CHW[0])
    assert sw > 0 and np.log2(sw) == np.rint(np.log2(sw))
    kind, g = sc.geom_of(sc.LAYERS, sc.SIZES, 0)
    W = sc.dense_weights(kind, g, p).astype(np.float32)
    x1, x2, r = fm16.split2(x, fm16.SX)
    w1, w2, rw = fm16.split2(W, sw)
    assert not x2.any() and not r.any() and not w2.any() and not rw.any()
    assert (np.abs(w1) == np.rint(np.abs(w1))).all() and np.abs(w1).max() <= 2 ** 14
    for a in (x, W):
        a1, a2, a3 = split3(a)
        assert np.array_equal(a1, a) and not a2.any() and not a3.any()
    b, _, _ = sc.int_params(p)
    pt = sc._patches(x1.transpose(0, 2, 3, 1).astype(np.float64), g).reshape(5, 19, 19, -1)
    out = pt @ w1.reshape(96, -1).astype(np.float64).T / (fm16.SX * sw) + b
    assert np.array_equal(out, ref["fm"][1][:5])


def test_mistakes_would_be_visible(ref):
    """Conditions, not measurements: every image's last-FC row differs from every other image's; each ReLU map has 20 - 70 % zeros;
    every image has a zero and a non-zero in every chunk of 16 channels of every ReLU map."""
    assert len({r.tobytes() for r in ref["rows"]}) == N
    for l in sc.RELUS:
        y = ref["fm"][l + 1]
        share = float((y == 0).mean())
        print("ReLU %d: %.1f %% zeros" % (l, 100 * share))
        assert 0.20 <= share <= 0.70, (l, share)
        ch = y.reshape(N, -1, y.shape[-1] // 16, 16)
        zero, live = (ch == 0).any(axis=(1, 3)), (ch != 0).any(axis=(1, 3))
        assert zero.all() and live.all(), l


def changed(ref, first, variant, n=N):
    """Does the mistake `variant` (sched_cases.forward_int) change the last-FC row of EVERY one of the first n images?"""
    out = sc.forward_int(ref["fm"][first][:n], first=first, variant=variant)[-1].reshape(n, -1)
    return bool((out != ref["rows"][:n]).any(axis=1).all())


def test_teeth_panels_sub_batches_and_chunks(ref):
    """An image that takes the input or an intermediate map of the image 128 further on ends with THAT image's row (the layers behind
    are per image); panels [p0, p1) of a sub-batch that keep the previous forward's values hold the rows of the images STEP * k
    further on (the GPU tier rotates the batch from forward to forward); a chunk written at panel 0 instead of pa leaves panels
    [pa, pb) with the previous forward's rows and panel 0 with another panel's.  All rows are distinct, so each of these differs
    in every image it touches — for every cut `panels * k / ns` of the grid."""
    rows = ref["rows"]
    assert (rows[:N - 128] != rows[128:]).any(axis=1).all()
    step, cuts = 131, set()
    for n, cfg, host in sc.grid():
        for pa, pb in sc.chunks(n, cfg["chunk"], host):
            cuts.update((n, p0, p1) for p0, p1 in sc.sub_batches(pa, pb, cfg["streams"]))
            if pa > 0:                                     # the chunk lands on panel 0: its own panels keep the last forward's rows
                lo, hi = pa * 128, min(n, pb * 128)
                assert (rows[lo:hi] != rows[(np.arange(lo, hi) + step) % N]).any(axis=1).all()
                assert (rows[:hi - lo] != rows[lo:hi]).any(axis=1).all()
    assert (3, 0, 1) in {(pb, p0, p1) for n, p0, p1 in cuts for pb in [-(-n // 128)]} and len(cuts) > 60
    for n, p0, p1 in cuts:
        idx = np.arange(p0 * 128, min(n, p1 * 128))
        for k in (1, 2, 5):
            assert (rows[idx] != rows[(idx + k * step) % N]).any(axis=1).all(), (n, p0, p1)
    assert sc.sub_batches(0, 3, 2) == [(0, 1), (1, 3)] and sc.sub_batches(0, 5, 3) == [(0, 1), (1, 3), (3, 5)]
    assert sc.sub_batches(0, 9, 4) == [(0, 2), (2, 4), (4, 6), (6, 9)] and sc.sub_batches(6, 7, 4) == [(6, 7)]
    assert sc.chunks(1027, 2) == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 9)] and sc.chunks(385, 2) == [(0, 4)] and sc.chunks(385, 1) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert sc.chunks(1027, 2, host=False) == [(0, 9)]


def test_teeth_fc_slices_bias_flatten(ref):
    """One slice of an FC layer's sub-space axis left out or added twice (2 to 4 slices, every slice), the bias added once per slice,
    the flatten in NHWC order: each changes every image's last-FC row."""
    prm = sc.params()
    for l in (8, 11, 13):
        kind, g = sc.geom_of(sc.LAYERS, sc.SIZES, l)
        M, _, Cs = sc.QUANT[l][:3]
        b, _, _ = sc.int_params(prm[l])
        for Z in (2, 3, 4):
            per = -(-M // Z)
            for z in range(Z):
                def part(x, lo=z * per * Cs, hi=min(M, (z + 1) * per) * Cs):
                    xf = sc.flatten_nchw(x).copy()
                    xf[:, :lo] = 0
                    xf[:, hi:] = 0
                    return sc.fc_int(xf, g, prm[l], bias=False).reshape(N, 1, 1, -1)
                assert changed(ref, l, {l: lambda l_, x, y: y - part(x)}), (l, Z, z, "left out")
                assert changed(ref, l, {l: lambda l_, x, y: y + part(x)}), (l, Z, z, "twice")
            assert changed(ref, l, {l: lambda l_, x, y: y + (Z - 1) * b}), (l, Z, "bias per slice")
    _, g8 = sc.geom_of(sc.LAYERS, sc.SIZES, 8)
    assert changed(ref, 8, {8: lambda l_, x, y: sc.fc_int(x.reshape(N, -1), g8, prm[8]).reshape(N, 1, 1, -1)}), "NHWC flatten"


def test_teeth_conv_slices_and_relu(ref):
    """One slice of a split conv tile left out or added twice — a slice is a run of the tile's (pixel, sub-space) stage sequence, here
    the upper / lower half of the source rows, in every tile (the planner splits from tile 0 on) and in the first 2 x 3 tile alone
    —, the bias added once per slice, the ReLU behind a conv / FC layer missing: each changes every image's last-FC row.  (The conv
    layers are recomputed for the first 259 images of the batch — two panels and a ragged third —, the FC-level mistakes for all.)"""
    prm = sc.params()
    n = 259
    for l in (3, 5):
        _, g = sc.geom_of(sc.LAYERS, sc.SIZES, l)
        b, _, _ = sc.int_params(prm[l])

        def part(x, rows):
            xm = np.zeros_like(x)
            xm[:, rows] = x[:, rows]
            return sc.conv_int(xm, g, prm[l], bias=False)

        def tile(x, y):
            out = y.copy()
            out[:, :2, :3] -= part(x, slice(0, 2))[:, :2, :3]
            return out
        assert changed(ref, l, {l: lambda l_, x, y: y - part(x, slice(0, 5))}, n), (l, "slice 0 of 2 left out")
        assert changed(ref, l, {l: lambda l_, x, y: y + part(x, slice(5, 10))}, n), (l, "slice 1 of 2 twice")
        assert changed(ref, l, {l: lambda l_, x, y: tile(x, y)}, n), (l, "one tile")
        assert changed(ref, l, {l: lambda l_, x, y: y + b}, n), (l, "bias per slice")
    for l in sc.RELUS:
        assert changed(ref, l, {l: lambda l_, x, y: x}, n if l < sc.FIRST_FC else N), (l, "ReLU missing")


# ---------------------------------------------------------------------------------------------- planner reach
def test_sched_reach_is_the_planner_answer():
    """Every launch of every forward of the grid — (panels, nsub, concurrent, in place, small, live, options) — through
    qcnn_plan_conv_query / qcnn_plan_fc_query: SCHED_REACH holds exactly these launches and the planner's answers."""
    pl = sc.Planner()
    keys = sc.grid_keys()
    assert keys == sorted(sc.SCHED_REACH)
    for k in keys:
        assert sc.predict(k, pl) == sc.SCHED_REACH[k], k
    # what qcnn_get_layer_split reports is the LAST launch's: the last sub-batch of the last chunk
    assert sc.launches_of(1027, sc.config())[-1][:3] == (1, 1, 0) and sc.launches_of(1027, sc.config(streams=4, chunk=0))[-1][:3] == (3, 4, 9)
    assert sc.launches_of(385, sc.config(chunk=1)) == [(1, 1, 0, 1, 0, 128, 1, 1, 1, 1)] * 4


def test_sched_reach_reaches_every_family():
    """Over the grid the LAST launches (the ones the GPU tier can see) contain: a tile launch with split tiles and one without, a split
    eight-wave launch, a sliding form, an eight-wave form, two families for one conv layer at different batch sizes, an FC layer with
    one and with several slices, k_fc_sym8, the decoded FC, the few-image kernels, the first layer in place and in panel form."""
    last = {sc.launches_of(n, cfg, host)[-1] for n, cfg, host in sc.grid()}
    rows = [sc.SCHED_REACH[k] for k in last]
    conv2, conv3 = {r[1] for r in rows}, {r[2] for r in rows}
    split_on = [sc.SCHED_REACH[k] for k in last if k[6] == 1 and k[7] == 1 and not k[4]]
    assert any(f >= 0 and z > 1 for f, z in conv2 | conv3)                              # split tiles (first split tile 0)
    assert any(r[2] == (-1, 1) for r in split_on)                                       # whole tiles, the split switched on
    assert any(f == -5 and z > 1 for f, z in conv2)                                     # split eight-wave launch
    assert any(f in (-2, -6, -10) and z >= 2 for f, z in conv2 | conv3)                  # a sliding form, two segments
    assert any(f in (-5, -9) for f, z in conv2 | conv3)
    for fams in (conv2, conv3):                                                         # the planner really chooses, per batch size
        assert len({f if f < 0 else "split" for f, z in {r for r in fams if r != (-11, 1)}}) >= 3, fams
    fc1 = {r[3] for r in rows}
    assert (-1, 1) in fc1 and any(z > 1 for f, z in fc1) and any(f == -5 for f, z in fc1)
    assert {r[4] for r in rows} >= {(-3, 1), (-1, 3), (-11, 1)}                          # decoded FC; 12-wave and few-image without it
    assert any(all(c == (-11, 1) for c in r) for r in rows)
    assert {r[0] for r in rows} >= {(-3, 2), (-3, 1), (-11, 1), (-1, 1)}                 # in place, panel form, few-image, table kernel
    assert any(k[3] and sc.SCHED_REACH[k][0] == (-1, 1) for k in last)                  # the tile kernel reads NCHW in place too
