"""CPU tier of the streamed 8-bit path: tests/stream_ref.py (the hit rule the GPU tests hold k_top5_hits to) against hand-made
rows and against eight single mistakes built into copies of it, and engine.split_batches.  No GPU."""
import numpy as np
import pytest

import layout_ref as lr
import stream_ref as sr
from conftest import pkg

engine = pkg("engine")


# ---------------------------------------------------------------------------------------------- the hit rule by hand
def test_a_label_at_each_rank_and_absent():
    row = [40, 7, 300, 0, 999]
    for r in range(5):
        want = [0] * 5
        want[r] = 1
        assert sr.hits5([row], [row[r]]).tolist() == want
    assert sr.hits5([row], [5]).tolist() == [0] * 5
    assert sr.hits5([row] * 3, [40, 5, 999]).tolist() == [1, 0, 0, 0, 1]
    assert sr.hits5(np.zeros((0, 5), np.uint16), np.zeros(0, np.uint16)).tolist() == [0] * 5
    assert sr.hits5([row], [40]).dtype == np.uint64


def test_a_row_of_five_equal_classes_counts_at_every_rank():
    assert sr.hits5([[9] * 5], [9]).tolist() == [1] * 5
    assert sr.hits5([[9] * 5], [8]).tolist() == [0] * 5
    assert sr.hits5([[3, 9, 3, 9, 3]], [3]).tolist() == [1, 0, 1, 0, 1]


def test_label_zero_against_the_references_repeated_zero_rows():
    """Fewer than five probabilities above FLT_MIN: the reference's sweeps fall back to class 0 again and again."""
    rows = [[17, 4, 0, 0, 0], [0, 0, 0, 0, 0], [17, 0, 4, 0, 0]]
    assert sr.hits5(rows, [0, 0, 0]).tolist() == [1, 2, 2, 3, 3]
    assert sr.hits5(rows, [17, 1, 4]).tolist() == [1, 0, 1, 0, 0]


def test_batches_skip_the_unlabelled_and_accumulate():
    a, b = [[1, 2, 3, 4, 5], [5, 4, 3, 2, 1]], [[7, 7, 7, 7, 7]]
    assert sr.hits5_batches([a, b, a], [[1, 1], None, [3, 3]]).tolist() == [1, 0, 2, 0, 1]
    assert sr.hits5_batches([a, b], [None, [7]], start=[10, 0, 0, 0, 2 ** 40]).tolist() == [11, 1, 1, 1, 2 ** 40 + 1]
    assert sr.accuracy([1, 0, 2, 0, 1], 4) == [0.25, 0.25, 0.75, 0.75, 1.0]


# ---------------------------------------------------------------------------------------------- eight wrong copies
V = 3          # views per image of the slot-indexed mistake


def _loop(top5, labels, n=None, label_of=lambda i: i, rank_to=lambda r: r, match=lambda row, lab: [int(x) == lab for x in row]):
    top5, labels = np.asarray(top5), np.asarray(labels)
    out = np.zeros(5, np.uint64)
    for i in range(top5.shape[0] if n is None else n(top5.shape[0])):
        m = match(top5[i], int(labels[label_of(i) % len(labels)]))
        for r in range(5):
            if m[r]:
                out[rank_to(r)] += np.uint64(1)
    return out


def _first_only(row, lab):
    m = [int(x) == lab for x in row]
    return [v and not any(m[:r]) for r, v in enumerate(m)]


def _last_only(row, lab):
    m = [int(x) == lab for x in row]
    return [v and not any(m[r + 1:]) for r, v in enumerate(m)]


def _batches(one=sr.hits5, skip_unlabelled=True, accumulate=True):
    def f(top5s, labels):
        out = np.zeros(5, np.uint64)
        for t, l in zip(top5s, labels):
            if l is None:
                if skip_unlabelled:
                    continue
                l = np.zeros(len(t), np.uint16)
            out = out + one(t, l) if accumulate else one(t, l)
        return out
    return f


MISTAKES = {
    "cumulative_instead_of_per_rank": _batches(lambda t, l: np.cumsum(sr.hits5(t, l)).astype(np.uint64)),
    "first_match_only": _batches(lambda t, l: _loop(t, l, match=_first_only)),
    "duplicates_counted_once": _batches(lambda t, l: _loop(t, l, match=_last_only)),
    "labels_indexed_per_slot": _batches(lambda t, l: _loop(t, l, label_of=lambda i: i * V)),
    "off_by_one_rank": _batches(lambda t, l: _loop(t, l, rank_to=lambda r: min(r + 1, 4))),
    "dropped_last_image": _batches(lambda t, l: _loop(t, l, n=lambda n: n - 1)),
    "unlabelled_batch_counted_against_class_0": _batches(skip_unlabelled=False),
    "counters_of_the_last_batch_only": _batches(accumulate=False),
}


def _crafted():
    """Batches on which every mistake above shows: hits at every rank, rows that repeat a class, an unlabelled batch whose
    rows hold class 0, a hit on the last image of a batch, more than one labelled batch."""
    rng = np.random.default_rng(41)
    rows = lambda n: np.stack([rng.permutation(20)[:5] + 1 for _ in range(n)]).astype(np.uint16)
    a, b, c = rows(7), rows(4), rows(5)
    la = np.array([a[0, 0], a[1, 1], a[2, 2], a[3, 3], a[4, 4], 50, a[6, 2]], np.uint16)      # every rank once, one miss, a hit on the last image
    b[:, 3] = 0                                                                                # the unlabelled batch holds class 0
    c[1] = [6, 6, 9, 6, 9]                                                                     # repeats
    c[4] = [2, 3, 2, 2, 2]
    lc = np.array([c[0, 1], 6, 50, c[3, 0], 2], np.uint16)
    return [a, b, c], [la, None, lc]


def test_the_reference_rule_on_the_crafted_batches():
    top5s, labels = _crafted()
    assert sr.hits5_batches(top5s, labels).tolist() == [1 + 1 + 1 + 1, 1 + 1 + 1, 1 + 1 + 1, 1 + 1 + 1, 1 + 1]


def test_the_mistakes_are_eight_and_named():
    assert len(MISTAKES) == 8
    for name in ("cumulative", "first_match", "duplicates", "per_slot", "off_by_one", "dropped_last"):
        assert any(name in k for k in MISTAKES), name


@pytest.mark.parametrize("name", sorted(MISTAKES))
def test_every_single_mistake_is_caught(name):
    top5s, labels = _crafted()
    want = sr.hits5_batches(top5s, labels)
    assert np.array_equal(_batches()(top5s, labels), want)                      # the scaffold itself restates the rule
    got = MISTAKES[name](top5s, labels)
    assert got.shape == (5,) and not np.array_equal(got, want), name


# ---------------------------------------------------------------------------------------------- split_batches
def _images(n, seed=42):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (3, 2 + k % 5, 3 + k % 4), dtype=np.uint8) for k in range(n)]


@pytest.mark.parametrize("n,max_batch,n_views", [(23, 40, 10), (23, 40, 1), (8, 40, 10), (5, 7, 3), (1, 1, 1), (12, 39, 10)])
def test_split_batches_caps_keeps_order_and_labels(n, max_batch, n_views):
    imgs = _images(n)
    labels = [(7 * k + 3) % 65536 for k in range(n)]
    cut = engine.split_batches(imgs, labels, max_batch, n_views)
    per = max_batch // n_views
    assert [len(d) for _, d, _ in cut] == [per] * (n // per) + ([n % per] if n % per else [])      # ragged last batch only
    assert all(len(d) * n_views <= max_batch for _, d, _ in cut)
    k = 0
    for flat, descs, lab in cut:
        assert flat.dtype == np.uint8 and flat.ndim == 1 and lab.dtype == np.uint16 and lab.shape == (len(descs),)
        for d, l in zip(descs, lab):
            assert np.array_equal(flat[d.sample_index(3)], imgs[k]) and int(l) == labels[k]      # order kept, the label follows its image
            k += 1
    assert k == n


def test_split_batches_of_bmp_files_and_without_labels():
    imgs = _images(7, seed=43)
    files = [lr.bmp24_file(a) if k % 2 else lr.bmp32_topdown_file(a) for k, a in enumerate(imgs)]
    cut = engine.split_batches(files, None, 9, 3)
    assert [len(d) for _, d, _ in cut] == [3, 3, 1] and all(l is None for _, _, l in cut)
    assert bytes(cut[1][0]) == b"".join(files[3:6])                                # the files untouched, back to back
    got = [flat[d.sample_index(3)] for flat, descs, _ in cut for d in descs]
    assert all(np.array_equal(g, a) for g, a in zip(got, imgs))


def test_split_batches_refuses():
    imgs = _images(3)
    with pytest.raises(ValueError):
        engine.split_batches([], [], 40, 10)
    with pytest.raises(ValueError):
        engine.split_batches(imgs, [1, 2], 40, 10)                                  # a label short
    with pytest.raises(ValueError):
        engine.split_batches(imgs, [1, 2, 70000], 40, 10)
    with pytest.raises(ValueError):
        engine.split_batches(imgs, [1, -2, 3], 40, 10)
    with pytest.raises(ValueError):
        engine.split_batches(imgs, None, 9, 10)                                     # no image fits
    with pytest.raises(ValueError):
        engine.split_batches(imgs, None, 9, 0)
    with pytest.raises(ValueError):
        engine.split_batches([imgs[0], lr.bmp24_file(imgs[1])], None, 9, 1)         # two kinds
