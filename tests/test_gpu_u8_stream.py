"""8-bit source batches streamed from host memory (qcnn_forward_u8_resized_host_batches / _relaxed_host_batches) and the device-side
hit counters (k_top5_hits, qcnn_count_top5_hits).

  * every batch of a stream bit for bit against ONE qcnn_forward_u8_*_views_strided call per batch on a second engine with the same
    options: the pass-through network (one ReLU on a (3, 5, 7) input, full image 12 x 14: the output is the packed input, so every
    source byte of every batch shows) with max_batch 270, and the tiny model (24 classes, golden parameters, LUT_MFMA) with 40;
  * buffer reuse: the largest and the smallest batch alternating, the call twice in a row and behind an un-synchronised forward;
  * pageable, pinned and registered source memory; outputs that were not asked for stay untouched;
  * hit counts through the stream and alone, exactly equal to tests/stream_ref.py;
  * refusals: non-zero, the batch named, every output and the counters untouched, the next good call right."""
import functools

import numpy as np
import pytest
import torch

import layout_ref as lr
import relaxed_ref as xr
import resize_ref as rr
import stream_ref as sr
import views_ref as vr
from conftest import pkg, tiny_params_from_golden
from u8_harness import DEV, Outputs, bits_equal, make_engine

pytestmark = pytest.mark.gpu

topo = pkg("topology")
capi = pkg("capi")
engine = pkg("engine")

PACK_CHW, FULL = (3, 5, 7), rr.FULL_HW
TINY_FULL = (40, 40)
METHOD = {"strict": "forward_u8_resized_views_strided_dev", "relaxed": "forward_u8_relaxed_views_strided_dev"}
# source sizes legal in both modes (two pixels a side) under which every ten-crop view stays inside every image
SIZES = {"pack": [(12, 14), (30, 8), (2, 2), (37, 53), (14, 54), (5, 100), (24, 27)],
         "tiny": [(14, 54), (30, 8), (2, 2), (37, 53), (100, 75), (5, 100), (40, 40)]}
LAYOUTS = ["planar", "bmp24", "bgr", "bmp32_topdown", "roi", "bgra_pitched", "rgb", "planar_pitched"]    # mixed inside every batch
# images per batch.  One view: the slots are the images — 1 and 3 (few-image kernels), 5, 127 / 128 / 129 (the panel seam), 270
# (max_batch, a ragged third panel).  Ten views: the slots are multiples of ten — 10, 120 / 130 (either side of the seam), 270,
# 20, 260, 50.  The tiny model (max_batch 40) likewise: 1, 3, 5, 40, 2, 39, 7 and 10, 40, 20, 30, 10, 40, 20 slots.
COUNTS = {("pack", 1): [1, 3, 5, 127, 128, 129, 270], ("pack", 10): [1, 12, 13, 27, 2, 26, 5],
          ("tiny", 1): [1, 3, 5, 40, 2, 39, 7], ("tiny", 10): [1, 4, 2, 3, 1, 4, 2]}


def _views(net, mode, V):
    full, (_, h, w) = (FULL, PACK_CHW) if net == "pack" else (TINY_FULL, topo.tiny_model()[0])
    if mode == "strict":
        return vr.ten_crop(full[0], full[1], h, w) if V == 10 else [((full[0] - h) // 2, (full[1] - w) // 2, 0)]
    return xr.ten_crop_anchored() if V == 10 else [xr.CENTRE]


def _mean(net, mode, seed):
    full, chw = (FULL, PACK_CHW) if net == "pack" else (TINY_FULL, topo.tiny_model()[0])
    shape = (3,) + tuple(full) if mode == "strict" else tuple(chw)
    return (np.random.default_rng(seed).standard_normal(shape) * 20 + 110).astype(np.float32)


@pytest.fixture(scope="module")
def engines(golden_tiny):
    """Per network two engines with the same options: [0] streams, [1] makes the per-batch references."""
    in_chw, layers = topo.tiny_model()
    params = tiny_params_from_golden(golden_tiny, layers)
    made = {"pack": [make_engine(PACK_CHW, [topo.relu()], {}, 270) for _ in range(2)],
            "tiny": [make_engine(in_chw, layers, params, 40, lut=capi.LUT_MFMA) for _ in range(2)]}
    yield made
    for pair in made.values():
        for e in pair:
            e.close()


@functools.lru_cache(maxsize=None)
def _buffers(net, counts, seed):
    """One lr.Buffer per batch: sizes cycling over the network's sources, layouts mixed inside every batch, all contents distinct."""
    out = []
    for b, n in enumerate(counts):
        rng = np.random.default_rng(seed + 17 * b)
        out.append(lr.Buffer(rr.random_images(rng, n, 3, SIZES[net]), LAYOUTS[b % 3:] + LAYOUTS[:b % 3], lr.rng_fill(seed + 17 * b + 1)))
    return out


class Mean:
    def __init__(self, mean):
        self.t = torch.from_numpy(np.ascontiguousarray(mean)).to(DEV) if mean is not None else None
        torch.cuda.synchronize()
        self.ptr = self.t.data_ptr() if self.t is not None else None


def per_batch(eng, mode, full, bufs, mean, views):
    """One strided device call per batch: [(prob, top5, rows)]."""
    out = []
    for buf in bufs:
        d = torch.from_numpy(buf.flat).to(DEV)
        o = Outputs(eng, len(buf.descs), len(views))
        torch.cuda.synchronize()
        getattr(eng, METHOD[mode])(d.data_ptr(), buf.flat.size, buf.descs, full[0], full[1], mean.ptr, views, *o.ptrs())
        eng.sync()
        out.append(o.host())
    return out


def fresh_outs(eng, counts, V, wants=(True, True, True)):
    """Host outputs per batch, pre-filled with NaN / 0xFFFF; wants: one triple for all batches or one per batch."""
    h, w, c = eng.fm_dims(eng.L)
    classes = h * w * c
    wants = [wants] * len(counts) if isinstance(wants[0], bool) else wants
    return [(np.full((n, classes), np.nan, np.float32) if wt[0] else None, np.full((n, 5), 0xFFFF, np.uint16) if wt[1] else None,
             np.full((n, V, classes), np.nan, np.float32) if wt[2] else None) for n, wt in zip(counts, wants)]


def untouched(outs):
    return all((p is None or np.isnan(p).all()) and (t is None or (t == 0xFFFF).all()) and (r is None or np.isnan(r).all()) for p, t, r in outs)


def stream(eng, mode, full, bufs, mean, views, wants=(True, True, True), flats=None, labels=None, hits5=None):
    outs = fresh_outs(eng, [len(b.descs) for b in bufs], len(views), wants)
    flats = [b.flat for b in bufs] if flats is None else flats
    eng.forward_u8_host_batches_into([(f, b.descs) for f, b in zip(flats, bufs)], full, mean.ptr, views, mode, outs, labels, hits5)
    return outs


def assert_equal_per_batch(got, want, what=""):
    assert len(got) == len(want)
    for b, ((p, t, r), (wp, wt, wr)) in enumerate(zip(got, want)):
        assert np.isfinite(wr).all()
        assert bits_equal(r.reshape(wr.shape), wr), "%s batch %d: prob_views differ" % (what, b)
        assert bits_equal(p, wp), "%s batch %d: prob differs" % (what, b)
        assert np.array_equal(t, wt), "%s batch %d: top5 differs" % (what, b)


@functools.lru_cache(maxsize=None)
def _case(net, mode, V):
    return _buffers(net, tuple(COUNTS[net, V]), 800 + V), _views(net, mode, V), _mean(net, mode, 801 + V)


def _run_case(engines, net, mode, V):
    bufs, views, mean = _case(net, mode, V)
    full = FULL if net == "pack" else TINY_FULL
    m = Mean(mean)
    want = per_batch(engines[net][1], mode, full, bufs, m, views)
    got = stream(engines[net][0], mode, full, bufs, m, views)
    assert_equal_per_batch(got, want, "%s %s V=%d" % (net, mode, V))
    return bufs, want


# ---------------------------------------------------------------------------------------------- 1. equals batch by batch
@pytest.mark.parametrize("V", [1, 10])
@pytest.mark.parametrize("mode", ["strict", "relaxed"])
@pytest.mark.parametrize("net", ["pack", "tiny"])
def test_stream_equals_one_strided_call_per_batch(engines, net, mode, V):
    bufs, want = _run_case(engines, net, mode, V)
    assert len(bufs) >= 7 and len({b.flat.tobytes() for b in bufs}) == len(bufs)
    assert all(len(set(b.layouts)) >= min(3, len(b.layouts)) for b in bufs)                  # mixed layouts inside a batch
    assert all(len({r.shape for r in b.refs}) >= min(3, len(b.refs)) for b in bufs)          # differing sizes inside a batch
    if net == "pack":                                                                        # the output IS the packed input
        assert len({w[2].tobytes() for w in want}) == len(want)


# ---------------------------------------------------------------------------------------------- 2. buffer reuse
@pytest.mark.parametrize("mode", ["strict", "relaxed"])
def test_buffers_are_reused_while_their_neighbour_is_in_flight(engines, mode):
    """big, 1-image, big, 1-image, ...: each device buffer and each pinned pair is rewritten four times, by batches whose
    src_bytes differ more than twenty-fold; then twice in a row, then behind an un-synchronised forward."""
    eng, ref = engines["pack"]
    counts = (27, 1, 26, 1, 27, 1, 25, 1, 27)
    bufs = _buffers("pack", counts, 820)
    sizes = [b.flat.size for b in bufs]
    assert min(sizes[0::2]) > 20 * max(sizes[1::2]) and len({b.flat.tobytes() for b in bufs}) == len(bufs)
    views, m = _views("pack", mode, 10), Mean(_mean("pack", mode, 821))
    want = per_batch(ref, mode, FULL, bufs, m, views)
    assert_equal_per_batch(stream(eng, mode, FULL, bufs, m, views), want, "first")
    a = stream(eng, mode, FULL, bufs, m, views)
    b = stream(eng, mode, FULL, bufs[::-1], m, views)                     # no sync of the caller's between the two
    assert_equal_per_batch(a, want, "second")
    assert_equal_per_batch(b, want[::-1], "reversed")
    x = torch.randn((270,) + PACK_CHW, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    eng.forward_dev(x.data_ptr(), 270)                                    # un-synchronised: the stream starts behind it
    assert_equal_per_batch(stream(eng, mode, FULL, bufs, m, views), want, "behind forward_dev")


# ---------------------------------------------------------------------------------------------- 3. host memory kinds, outputs not asked for
def test_pageable_pinned_and_registered_sources_give_the_same_bits(engines):
    eng, ref = engines["pack"]
    bufs, views, mean = _case("pack", "strict", 10)
    m = Mean(mean)
    want = per_batch(ref, "strict", FULL, bufs, m, views)
    pinned = [engine.host_alloc(b.flat.size) for b in bufs]
    registered = [b.flat.copy() for b in bufs]
    try:
        for p, r, b in zip(pinned, registered, bufs):
            p[:] = b.flat
            engine.host_register(r)
        for kind, flats in (("pageable", None), ("pinned", pinned), ("registered", registered)):
            assert_equal_per_batch(stream(eng, "strict", FULL, bufs, m, views, flats=flats), want, kind)
    finally:
        for p, r in zip(pinned, registered):
            engine.host_free(p)
            engine.host_unregister(r)


def test_outputs_not_asked_for_stay_untouched(engines):
    eng, ref = engines["pack"]
    bufs, views, mean = _case("pack", "relaxed", 10)
    m = Mean(mean)
    want = per_batch(ref, "relaxed", FULL, bufs, m, views)
    triples = [(True, False, False), (False, True, False), (False, False, True), (False, False, False), (True, True, False),
               (True, False, True), (False, True, True)]
    counts = [len(b.descs) for b in bufs]
    outs = fresh_outs(eng, counts, 10)                                    # all arrays exist; only the asked-for ones are handed over
    given = [tuple(a if w else None for a, w in zip(o, wt)) for o, wt in zip(outs, triples)]
    eng.forward_u8_host_batches_into([(b.flat, b.descs) for b in bufs], FULL, m.ptr, views, "relaxed", given)
    for b, (o, wt, w) in enumerate(zip(outs, triples, want)):
        for j, name in enumerate(("prob", "top5", "prob_views")):
            if wt[j]:
                same = np.array_equal(o[j], w[j]) if j == 1 else bits_equal(o[j].reshape(w[j].shape), w[j])
                assert same, "batch %d: %s differs" % (b, name)
            else:
                assert untouched([tuple(o[k] if k == j else None for k in range(3))]), "batch %d: %s was written" % (b, name)
    p, t, r, hits = eng.forward_u8_host_batches([(b.flat, b.descs) for b in bufs], FULL, mean, views, "relaxed")   # the wrapper's defaults
    assert r is None and hits is None and all(bits_equal(a, w[0]) for a, w in zip(p, want)) and all(np.array_equal(a, w[1]) for a, w in zip(t, want))


# ---------------------------------------------------------------------------------------------- 4. hits through the stream
def _craft_labels(top5, classes, first):
    """Per image a chosen rank of its own row (first + i) % 6: 0..4 that entry, 5 a class outside the row."""
    lab = np.empty(len(top5), np.uint16)
    for i, row in enumerate(top5):
        k = (first + i) % 6
        lab[i] = row[k] if k < 5 else next(c for c in range(classes) if c not in set(int(x) for x in row))
    return lab


@pytest.mark.parametrize("mode", ["strict", "relaxed"])
def test_hits_through_the_stream(engines, mode):
    eng, ref = engines["tiny"]
    bufs, views, mean = _case("tiny", mode, 10)
    blocking = ref.forward_u8_relaxed_host if mode == "relaxed" else ref.forward_u8_resized_host
    top5s = [blocking(None, TINY_FULL, mean, views, descs=(b.flat, b.descs))[1] for b in bufs]
    labels = [_craft_labels(t, 24, 3 * b) for b, t in enumerate(top5s)]
    labels[2] = labels[5] = None                                          # two batches are not counted
    assert all(l is None or l.shape == (len(b.descs),) for l, b in zip(labels, bufs))      # one label per image, ten slots each
    want = sr.hits5_batches(top5s, labels)
    assert want.sum() > 0 and (want > 0).sum() >= 4
    m = Mean(mean)
    hits = np.full(5, 2 ** 63 + 5, np.uint64)                             # overwritten, not added to
    outs = stream(eng, mode, TINY_FULL, bufs, m, views, wants=(False, True, False), labels=labels, hits5=hits)
    assert all(np.array_equal(o[1], t) for o, t in zip(outs, top5s))
    assert hits.tolist() == want.tolist()
    hits2 = np.zeros(5, np.uint64)                                        # counted without any host output asked for
    stream(eng, mode, TINY_FULL, bufs, m, views, wants=(False, False, False), labels=labels, hits5=hits2)
    assert hits2.tolist() == want.tolist()
    none = np.full(5, 7, np.uint64)                                       # no labelled batch: five zeros
    stream(eng, mode, TINY_FULL, bufs[:2], m, views, labels=[None, None], hits5=none)
    assert none.tolist() == [0] * 5


def test_evaluate_u8_returns_the_cumulative_fractions(engines):
    eng, ref = engines["tiny"]
    rng = np.random.default_rng(840)
    images = rr.random_images(rng, 11, 3, SIZES["tiny"])
    views, mean = _views("tiny", "strict", 10), _mean("tiny", "strict", 841)
    cut = engine.split_batches(images, None, 40, 10)
    assert [len(d) for _, d, _ in cut] == [4, 4, 3]
    top5 = np.concatenate([ref.forward_u8_resized_host(None, TINY_FULL, mean, views, descs=(f, d))[1] for f, d, _ in cut])
    labels = _craft_labels(top5, 24, 1)
    hits = sr.hits5(top5, labels)
    got = eng.evaluate_u8(images, labels, TINY_FULL, mean, views)
    assert got["n"] == 11 and got["hits"] == hits.tolist() and got["accuracy"] == sr.accuracy(hits, 11)
    assert got["accuracy"] == sorted(got["accuracy"]) and 0 < got["accuracy"][0] < got["accuracy"][4] < 1
    small = eng.evaluate_u8(images, labels, TINY_FULL, mean, views, batch_images=3)           # another cut: four batches
    assert small["n"] == 11 and len(small["hits"]) == 5


# ---------------------------------------------------------------------------------------------- 5. qcnn_count_top5_hits alone
def _count(eng, top5, labels, hits):
    d_t = torch.from_numpy(np.ascontiguousarray(top5).view(np.int16)).to(DEV)
    d_l = torch.from_numpy(np.ascontiguousarray(labels).view(np.int16)).to(DEV)
    torch.cuda.synchronize()
    eng.count_top5_hits_dev(d_t.data_ptr(), d_l.data_ptr(), len(labels), hits.data_ptr())
    eng.sync()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_count_top5_hits_alone(engines, n):
    eng = engines["pack"][0]
    rng = np.random.default_rng(850 + n)
    top5 = rng.integers(0, 12, (n, 5)).astype(np.uint16)                   # twelve classes: rows repeat classes
    top5[::3] += 60000                                                    # and the upper half of the 16 bits
    assert n < 60 or any(len(set(r)) < 5 for r in top5.tolist())
    labels = np.where(rng.random(n) < 0.5, top5[np.arange(n), rng.integers(0, 5, n)], rng.integers(0, 12, n)).astype(np.uint16)
    labels[-1] = top5[-1, 4]                                              # the last image hits: a dropped tail shows
    start = np.array([5, 0, 2 ** 40, 1, 2 ** 63], np.uint64)              # accumulated INTO non-zero counters, over three calls
    hits = torch.from_numpy(start.view(np.int64).copy()).to(DEV)
    cuts = [0, n // 3, n - n // 4, n]
    want = start.copy()
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            _count(eng, top5[a:b], labels[a:b], hits)
            want = want + sr.hits5(top5[a:b], labels[a:b])
    assert hits.cpu().numpy().view(np.uint64).tolist() == want.tolist()
    whole = torch.zeros(5, dtype=torch.int64, device=DEV)
    _count(eng, top5, labels, whole)
    assert whole.cpu().numpy().view(np.uint64).tolist() == sr.hits5(top5, labels).tolist()
    every = torch.zeros(5, dtype=torch.int64, device=DEV)                 # all hits: rows of five equal classes
    same = np.repeat(labels[:, None], 5, axis=1)
    _count(eng, same, labels, every)
    assert every.cpu().tolist() == [n] * 5
    nothing = torch.zeros(5, dtype=torch.int64, device=DEV)               # no hits
    _count(eng, top5, np.full(n, 30000, np.uint16), nothing)
    assert nothing.cpu().tolist() == [0] * 5


def test_count_top5_hits_refuses_null_and_empty(engines):
    eng = engines["pack"][0]
    hits = torch.zeros(5, dtype=torch.int64, device=DEV)
    t = torch.zeros((4, 5), dtype=torch.int16, device=DEV)
    l = torch.zeros(4, dtype=torch.int16, device=DEV)
    for args in ((None, l.data_ptr(), 4, hits.data_ptr()), (t.data_ptr(), None, 4, hits.data_ptr()), (t.data_ptr(), l.data_ptr(), 4, None),
                 (t.data_ptr(), l.data_ptr(), 0, hits.data_ptr())):
        with pytest.raises(engine.QcnnError):
            eng.count_top5_hits_dev(*args)
    eng.sync()
    assert hits.cpu().tolist() == [0] * 5


# ---------------------------------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("mode", ["strict", "relaxed"])
def test_refusals_leave_everything_untouched(engines, mode):
    eng = engines["pack"][0]
    bufs, views, mean = _case("pack", mode, 10)
    m = Mean(mean)
    counts = [len(b.descs) for b in bufs]
    good = [(b.flat, b.descs) for b in bufs]
    labels = [np.zeros(n, np.uint16) for n in counts]
    last = len(bufs) - 1

    def swap(k, descs=None, null_source=False):
        return good[:k] + [(None if null_source else good[k][0], good[k][1] if descs is None else descs)] + good[k + 1:]

    def relabel(k, i, value):
        out = [l.copy() for l in labels]
        out[k][i] = value
        return out

    beyond = bufs[last].descs[:-1] + [bufs[last].descs[-1]._replace(offset=bufs[last].flat.size)]
    leaves = [(FULL[0] - 4, 0, 0)] if mode == "strict" else [(2, 2, 1, 0, 0)]
    bad = [
        # (batches, views, labels, words of the message)
        (swap(last, descs=beyond), views, labels, ("batch %d" % last, "image %d" % (counts[last] - 1), "leave the source buffer")),
        (swap(3, descs=bufs[3].descs + bufs[3].descs[:1]), views, None, ("batch 3", "batch slots")),       # 28 x 10 = 280 > 270
        (good, views, relabel(4, 1, 105), ("batch 4", "image 1", "label 105")),                            # classes = 105
        (swap(2, null_source=True), views, labels, ("batch 2", "NULL")),
        ([], views, None, ("no batches",)),
        (good, leaves, labels, ("leaves",)),
        (swap(5, descs=[]), views, None, ("batch 5", "no image")),
    ]
    for batches, vws, labs, words in bad:
        outs = fresh_outs(eng, [len(d) for _, d in batches], 10)
        hits = np.array([11, 12, 13, 14, 2 ** 64 - 1], np.uint64)
        with pytest.raises(engine.QcnnError) as err:
            eng.forward_u8_host_batches_into(batches, FULL, m.ptr, vws, mode, outs, labs[:len(batches)] if labs is not None else None, hits)
        assert all(word in str(err.value) for word in words), (words, str(err.value))
        assert untouched(outs), "a refused call wrote an output (%r)" % (words,)
        assert hits.tolist() == [11, 12, 13, 14, 2 ** 64 - 1], "a refused call wrote the counters (%r)" % (words,)
    _run_case(engines, "pack", "strict", 1)                               # the same context then runs the first case
