"""Multi-view inference from 8-bit images (qcnn_forward_u8_views: k_pack_u8_views, the layers, k_mean_views) bit for bit
against tests/views_ref.py: the existing forward pass on crops and mirrors made on the host, at the same slot count in the same
slot order, and the fp32 averaging sequence.

  * the pack kernel per element on a glue-only network (fm[0] read back): element axis across the 64-element block, slots across
    panel seams and a ragged last panel, views at both far edges, odd offsets, mirrors, a repeated view, 1 / 3 / 32 views;
  * the whole path on the tiny network: per-view rows, averaged rows, top-5, fm[0]; one view = qcnn_forward_u8; three slots on
    the few-image kernels; NULL outputs; rejected arguments leave nothing behind; the scratch map grows;
  * the averaging kernel alone behind a soft-max layer, views that disagree on the winner, classes across the 128-class seam."""
import numpy as np
import pytest
import torch

import glue_ref as gr
import views_ref as vr
from conftest import pkg, tiny_params_from_golden
from u8_harness import DEV, Outputs, bits_equal, make_engine

pytestmark = pytest.mark.gpu

topo = pkg("topology")
capi = pkg("capi")
engine = pkg("engine")


def run_views(eng, px, mean, views, want_prob=True, want_top5=True, want_rows=True):
    """qcnn_forward_u8_views on device copies of px / mean -> (prob [n][classes], top5 [n][5], rows [n*V][classes]); None where
    the output was not asked for."""
    d_px = torch.from_numpy(px).to(DEV)
    d_mean = torch.from_numpy(mean).to(DEV) if mean is not None else None
    out = Outputs(eng, px.shape[0], len(views), (want_prob, want_top5, want_rows))
    torch.cuda.synchronize()
    eng.forward_u8_views_dev(d_px.data_ptr(), px.shape[2], px.shape[3], d_mean.data_ptr() if mean is not None else None,
                             px.shape[0], views, *out.ptrs())
    eng.sync()
    return out.host()


# ---------------------------------------------------------------------------------------------- 1. the pack kernel, per element
PACK_CHW, PACK_SRC = (3, 5, 7), (9, 12)           # E = 105: one full 64-element block and a tail of 41
TEN = vr.ten_crop(9, 12, 5, 7)
ODD = [(4, 5, 0), (1, 3, 1), (3, 1, 0), (1, 3, 1), (4, 5, 1), (0, 0, 1), (2, 5, 0)]      # the far corner, odd offsets, mirrors, a repeat


def _many_views(count, seed):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(0, 5)), int(rng.integers(0, 6)), int(rng.integers(0, 2))) for _ in range(count)]


def _position_mean():
    """A mean under which no two elements of a source image give the same value: 1000 x the element's index (exact in fp32)."""
    c, (hs, ws) = PACK_CHW[0], PACK_SRC
    return (np.arange(c * hs * ws, dtype=np.float32) * np.float32(1000)).reshape(c, hs, ws)


PACK_CASES = [
    # id, n, views, mean: 270 slots = two panels + 14, images 12 and 25 straddle a seam
    ("ten_crop", 27, TEN, "none"), ("ten_crop_mean", 27, TEN, "random"), ("ten_crop_unique", 27, TEN, "position"),
    ("odd", 27, ODD, "none"), ("odd_mean", 27, ODD, "random"),                  # 189 slots, image 18 straddles the seam
    ("one_view", 5, [(3, 4, 1)], "random"), ("one_view_plain", 131, [(4, 5, 0)], "none"),
    ("three_views", 45, [(0, 5, 1), (4, 0, 0), (2, 3, 1)], "random"),           # 135 slots, image 42 straddles the seam
    ("max_views", 5, _many_views(32, 71), "random"), ("max_views_plain", 5, _many_views(32, 72), "none"),   # 160 slots
]


@pytest.fixture(scope="module")
def pack_engine():
    eng = make_engine(PACK_CHW, [topo.relu()], {}, 270)
    yield eng
    eng.close()


@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: c[0])
def test_pack_per_element(pack_engine, case):
    _, n, views, mean_kind = case
    (c, h, w), (hs, ws) = PACK_CHW, PACK_SRC
    rng = np.random.default_rng(100 + n + len(views))
    px = rng.integers(0, 256, (n, c, hs, ws), dtype=np.uint8)
    mean = {"none": None, "random": (rng.standard_normal((c, hs, ws)) * 20 + 110).astype(np.float32),
            "position": _position_mean()}[mean_kind]
    want = vr.nhwc(vr.make_views(px, mean, views, h, w))
    if mean_kind == "position":
        assert all(np.unique(want[s]).size == want[s].size for s in range(want.shape[0]))
    _, _, rows = run_views(pack_engine, px, mean, views, want_prob=False, want_top5=False)
    got = pack_engine.layer_output(0, n * len(views))
    if not bits_equal(got, want):
        at = tuple(int(v) for v in np.argwhere(got.view(np.uint32) != want.view(np.uint32))[0])
        raise AssertionError("fm[0] differs in %d of %d elements; first at (slot, y, x, c) = %r (image %d, view %r): got %r, expected %r"
                             % (int((got.view(np.uint32) != want.view(np.uint32)).sum()), got.size, at, at[0] // len(views),
                                views[at[0] % len(views)], got[at], want[at]))
    assert bits_equal(rows, np.maximum(want, np.float32(0)).reshape(n * len(views), -1))     # the ReLU behind it, slot for slot


# ---------------------------------------------------------------------------------------------- 2. - 7. the whole path, tiny network
TINY_SRC = (40, 45)


class Tiny:
    """The tiny network with the golden parameters, MFMA builder, 130 batch slots; 13 source images of 40 x 45 under the ten-crop
    views, and the reference forward of their 130 host-made crops (computed once, never changed)."""

    def __init__(self, z):
        self.in_chw, self.layers = topo.tiny_model()
        self.params = tiny_params_from_golden(z, self.layers)
        c, h, w = self.in_chw
        rng = np.random.default_rng(77)
        self.px = rng.integers(0, 256, (13, c) + TINY_SRC, dtype=np.uint8)
        self.mean = (rng.standard_normal((c,) + TINY_SRC) * 20 + 110).astype(np.float32)
        self.views = engine.ten_crop_views(TINY_SRC[0], TINY_SRC[1], h, w)
        assert self.views == vr.ten_crop(TINY_SRC[0], TINY_SRC[1], h, w)
        self.eng = self.engine()
        self.crops = vr.make_views(self.px, self.mean, self.views, h, w)
        self.rows, _ = self.eng.forward_host(self.crops)                         # 130 images: the slot count of the views call
        self.fm0 = self.eng.layer_output(0, 130)
        self.prob = vr.mean_views(self.rows, 10)
        self.top5 = gr.top5(self.prob)

    def engine(self, max_batch=130):
        return make_engine(self.in_chw, self.layers, self.params, max_batch, lut=capi.LUT_MFMA)

    def check(self, eng, prob=True, top5=True, rows=True):
        got = run_views(eng, self.px, self.mean, self.views, prob, top5, rows)
        assert got[0] is None if not prob else bits_equal(got[0], self.prob)
        assert got[1] is None if not top5 else np.array_equal(got[1], self.top5)
        assert got[2] is None if not rows else bits_equal(got[2], self.rows)


@pytest.fixture(scope="module")
def tiny(golden_tiny):
    t = Tiny(golden_tiny)
    yield t
    t.eng.close()


def test_whole_path_ten_crop(tiny):
    assert np.isfinite(tiny.rows).all()
    prob, top5, rows = run_views(tiny.eng, tiny.px, tiny.mean, tiny.views)
    assert bits_equal(tiny.eng.layer_output(0, 130), tiny.fm0)
    assert bits_equal(rows, tiny.rows)
    assert bits_equal(prob, tiny.prob)
    assert np.array_equal(top5, tiny.top5)
    # a mirrored view is the mirror of the plain one, bit for bit
    fm0 = tiny.fm0.reshape(13, 10, *tiny.fm0.shape[1:])
    assert bits_equal(fm0[:, 5:], fm0[:, :5, :, ::-1])


def test_one_centre_view_is_forward_u8(tiny):
    n, (hs, ws) = 13, TINY_SRC
    centre = [tiny.views[4]]
    d_px, d_mean = torch.from_numpy(tiny.px).to(DEV), torch.from_numpy(tiny.mean).to(DEV)
    d_prob = torch.empty((n, tiny.rows.shape[1]), dtype=torch.float32, device=DEV)
    d_top5 = torch.empty((n, 5), dtype=torch.int16, device=DEV)
    torch.cuda.synchronize()
    tiny.eng.forward_u8_dev(d_px.data_ptr(), hs, ws, d_mean.data_ptr(), n, d_prob.data_ptr(), d_top5.data_ptr())
    tiny.eng.sync()
    fm0 = tiny.eng.layer_output(0, n)
    prob, top5, rows = run_views(tiny.eng, tiny.px, tiny.mean, centre)
    assert bits_equal(tiny.eng.layer_output(0, n), fm0)
    assert bits_equal(prob, d_prob.cpu().numpy()) and bits_equal(rows, prob)
    assert np.array_equal(top5, d_top5.cpu().numpy().view(np.uint16))


def test_one_image_three_views_on_the_few_image_kernels(tiny):
    views = [tiny.views[1], tiny.views[9], (3, 5, 0)]
    px = tiny.px[6:7]
    c, h, w = tiny.in_chw
    want_rows, _ = tiny.eng.forward_host(vr.make_views(px, tiny.mean, views, h, w))        # three images: the few-image kernels
    conv = [l for l, ly in enumerate(tiny.layers) if ly["type"] == topo.CONV][0]
    family = tiny.eng.layer_split(conv)
    prob, top5, rows = run_views(tiny.eng, px, tiny.mean, views)
    print("first conv layer at three slots: family code %r" % (family,))
    assert tiny.eng.layer_split(conv) == family                       # the same kernel family took both launches
    assert bits_equal(rows, want_rows)
    assert bits_equal(prob, vr.mean_views(want_rows, 3))
    assert np.array_equal(top5, gr.top5(vr.mean_views(want_rows, 3)))


@pytest.mark.parametrize("missing", ["prob", "top5", "rows"])
def test_null_outputs(tiny, missing):
    tiny.check(tiny.eng, prob=missing != "prob", top5=missing != "top5", rows=missing != "rows")


def test_rejections_launch_nothing(tiny):
    c, h, w = tiny.in_chw
    hs, ws = TINY_SRC
    eng = tiny.engine()
    tiny.check(eng)
    one = tiny.px[:1]
    bad = [
        (one, [(hs - h + 1, 0, 0)]),                          # oy + in_h > src_h
        (one, [(0, 0, 0), (0, -1, 0)]),                       # ox = -1
        (one, [(0, ws - w + 1, 1)]),                          # ox + in_w > src_w
        (one, [(-1, 0, 0)]),
        (one, []),                                            # no view
        (one, [(0, 0, 0)] * 33),                              # more than QCNN_MAX_VIEWS
        (np.zeros((131, c, hs, ws), np.uint8), [(0, 0, 0)]),  # max_batch + 1 slots
        (np.zeros((14, c, hs, ws), np.uint8), tiny.views),    # 140 slots
    ]
    for px, views in bad:
        with pytest.raises(engine.QcnnError):
            run_views(eng, px, tiny.mean, views)
        assert bits_equal(eng.layer_output(0, 130), tiny.fm0), "a rejected call wrote the input map"
    with pytest.raises(engine.QcnnError):                     # n = 0
        eng.forward_u8_views_dev(1, hs, ws, None, 0, [(0, 0, 0)])
    tiny.check(eng)
    eng.close()
    fresh = engine.QcnnEngine(0)                              # no model committed
    with pytest.raises(engine.QcnnError):
        fresh.forward_u8_views_dev(1, hs, ws, None, 1, [(0, 0, 0)])
    fresh.close()


def test_scratch_map_grows(tiny):
    """The averaged map is sized by the panels of n: one panel for 13 images, two for 130."""
    c, h, w = tiny.in_chw
    eng = tiny.engine()
    tiny.check(eng)
    rng = np.random.default_rng(78)
    px = rng.integers(0, 256, (130, c) + TINY_SRC, dtype=np.uint8)
    view = [(9, 0, 1)]
    want_rows, want_top5 = eng.forward_host(vr.make_views(px, tiny.mean, view, h, w))
    prob, top5, rows = run_views(eng, px, tiny.mean, view)
    assert bits_equal(rows, want_rows) and bits_equal(prob, want_rows) and np.array_equal(top5, want_top5)
    tiny.check(eng)                                           # and the small call again on the grown map
    eng.close()


# ---------------------------------------------------------------------------------------------- 8. the averaging kernel alone
@pytest.mark.parametrize("C", [3, 130])
def test_mean_views_behind_a_softmax(C):
    """A soft-max layer over C logits = pixel - 10.5; the three views are the three columns of a 1 x 3 source.  In every image
    view 0 puts its weight on one class and view 1 on another; 45 images = 135 slots, image 42 lies across the panel seam."""
    n, V = 45, 3
    views = [(0, 0, 0), (0, 1, 0), (0, 2, 0)]
    rng = np.random.default_rng(800 + C)
    px = rng.integers(0, 20, (n, C, 1, 3), dtype=np.uint8)
    for i in range(n):
        px[i, i % C, 0, 0] = 30                                # view 0: class i % C wins
        px[i, (i + 1 + (i // C) % (C - 1)) % C, 0, 1] = 30 + i % 2   # view 1: another class wins, every other image by more
    px[7, :, 0, 2] = px[7, :, 0, 0]                            # image 7: views 0 and 2 agree
    mean = np.full((C, 1, 3), 10.5, np.float32)
    eng = make_engine((C, 1, 1), [topo.smax()], {}, n * V)
    want_rows, _ = eng.forward_host(vr.make_views(px, mean, views, 1, 1))
    assert np.isfinite(want_rows).all()
    winners = want_rows.reshape(n, V, C).argmax(axis=2)
    assert (winners[:, 0] != winners[:, 1]).all()
    want = vr.mean_views(want_rows, V)
    prob, top5, rows = run_views(eng, px, mean, views)
    assert bits_equal(rows, want_rows)
    assert bits_equal(prob, want)
    assert np.array_equal(top5, gr.top5(want))
    # one view: the mean is the row itself
    prob1, top1, rows1 = run_views(eng, px, mean, views[1:2])
    want1, _ = eng.forward_host(vr.make_views(px, mean, views[1:2], 1, 1))
    assert bits_equal(rows1, want1) and bits_equal(prob1, want1) and np.array_equal(top1, gr.top5(want1))
    eng.close()
