"""The forward schedule held to exact sums: whatever run_layers, launch_conv, launch_fc, fc_input (qcnn_engine_run.hip) and the host
schedules (qcnn_engine_host.hip) decide for a batch, the exact network of tests/sched_cases.py must come out as the integer result
of a plain CPU computation, bit for bit — sub-batches on 1 to 4 streams (`panels * k / ns`: 3 panels on 2 streams run as 1 + 2), host
chunks with pa > 0 and a last chunk of fewer panels than streams, every sub-batch's share of the split-tile scratch, its FC partial
slab and its piece of the flatten scratch, the plan cache keyed by (panelsAll, panels, nsub, options), the planner's own cuts at every
batch size, ReLU fused into the conv / FC store and aliased maps, the first layer read in place from NCHW at panel0, the few-image
kernels.  No tolerance: every conv / FC assertion is np.array_equal (tests/test_sched_cases_cpu.py proves the data exact, the
mistakes visible and SCHED_REACH the planner's answer, without a GPU).

Every forward here
  * runs on other images than the forward before it (the batch rotated by a multiple of 131 images), so that a panel, a scratch
    slab or a map that keeps the previous forward's values holds ANOTHER image's numbers, and every image's last-FC row differs
    from every other image's;
  * asserts the last-FC map (and the second pool map in front of the first FC layer) equal to the integer result;
  * asserts the family code qcnn_get_layer_split reports for every conv / FC layer — the LAST launch of the forward: the last
    sub-batch of the last chunk — against sched_cases.SCHED_REACH;
  * holds the probabilities to the float64 soft-max of the integer logits within glue_ref.softmax_bound, the top-5 to glue_ref's rule
    applied to the device's own probabilities, and both bit-equal for the same image in every schedule: ten classes fit
    k_softmax_lds in every one of them (the batch only sets its grid: 32 images per workgroup), so every forward of this module
    runs the same soft-max arithmetic per image.
One engine is open at a time (LABBOOK.md, "Recorded plans of the launch planner": an unexplained fault with two engines open in one
process); options are set between forwards (qcnn_set_option has no commit-time state)."""
import numpy as np
import pytest

import glue_ref as gr
import sched_cases as sc
from conftest import pkg

pytestmark = pytest.mark.gpu

engine = pkg("engine")
N = sc.N_MAX
STEP = 131                 # images the batch is rotated by from one forward to the next
_state = dict(eng=None, forwards=0, prob=None, seen=None)


@pytest.fixture(scope="module")
def ref():
    """The integer result, computed once: dict(x, fm, logits64, p64, bound)."""
    x, fm, _ = sc.reference()
    logits = fm[sc.LAST_FC + 1].reshape(N, -1).astype(np.float64) * sc.unit(sc.LAST_FC + 1)
    p64 = gr.softmax64(logits)
    _state.update(prob=np.zeros((N, p64.shape[1]), np.float32), seen=np.zeros(N, bool))
    yield dict(x=x, fm=fm, want={l: sc.as_float32(fm[l], l) for l in (sc.FIRST_FC, sc.LAST_FC + 1)}, p64=p64, bound=gr.softmax_bound(p64))
    close_engine()


def close_engine():
    if _state["eng"] is not None:
        _state["eng"].close()
        _state["eng"] = None


def open_engine(in_chw=sc.IN_CHW, layers=sc.LAYERS, prm=None, max_batch=N):
    close_engine()
    eng = engine.QcnnEngine(0)
    eng.load_model(in_chw, layers, sc.file_params(prm or sc.params()), max_batch)
    _state["eng"] = eng
    return eng


def set_cfg(eng, cfg):
    for k, v in cfg.items():
        eng.set_option(sc.OPT[k], v)


def next_images(n):
    """Indices into THE batch of the next forward's n images: rotated on from the forward before."""
    _state["forwards"] += 1
    return (np.arange(n) + _state["forwards"] * STEP) % N


def equal(got, want, what):
    got = np.asarray(got).reshape(want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d of %d elements are not the integer result; first at %r: got %r, want %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), float(got[bad][0]), float(want[bad][0]))


def check_outputs(ref, idx, prob, top5, what):
    """prob / top5 of the images idx: the soft-max bound, the top-5 rule on the device's own rows, the same bits as in every schedule
    before."""
    gr.check_bound(prob, ref["p64"][idx], ref["bound"][idx], what + ": soft-max")
    if top5 is not None:
        gr.check_exact(np.asarray(top5).view(np.uint16).reshape(-1, 5), gr.top5(prob), what + ": top-5")
    seen = _state["seen"][idx]
    assert np.array_equal(prob[seen], _state["prob"][idx[seen]]), what + ": soft-max bits differ from another schedule's"
    _state["prob"][idx[~seen]] = prob[~seen]
    _state["seen"][idx] = True


def ensure_seen(eng, ref):
    """Every image's probabilities on record, from a forward whose logits were held to the integer result."""
    if not _state["seen"].all():
        _state["forwards"] = -1
        check_forward(eng, ref, N, sc.config())


def check_codes(eng, n, cfg, host, what):
    key = sc.launches_of(n, cfg, host)[-1]
    want = sc.reported(sc.SCHED_REACH[key])
    got = tuple(eng.layer_split(l) for l in sc.QLAYERS)
    assert got == want, "%s: layers %r ran %r, SCHED_REACH[%r] says %r" % (what, sc.QLAYERS, got, key, want)
    return got


def check_forward(eng, ref, n, cfg, every_map=False):
    """One forward_host of n images under cfg, every assertion of the module's docstring; every_map: all materialised maps."""
    what = "%d images, %r" % (n, {k: v for k, v in cfg.items() if v != sc.DEFAULTS[k]})
    set_cfg(eng, cfg)
    idx = next_images(n)
    prob, top5 = eng.forward_host(ref["x"][idx])
    codes = check_codes(eng, n, cfg, True, what)
    for l in (sc.LAST_FC + 1, sc.FIRST_FC):
        equal(eng.layer_output(l, n), ref["want"][l][idx], "%s: fm[%d]" % (what, l))
    if every_map:
        assert cfg["keep_all"] == 1
        for l in range(1, sc.LAST_FC + 2):
            equal(eng.layer_output(l, n), sc.as_float32(ref["fm"][l][idx], l), "%s: fm[%d]" % (what, l))
    check_outputs(ref, idx, prob, top5, what)
    return codes


# ---------------------------------------------------------------------------------------------- batch sizes x streams
@pytest.mark.parametrize("n", sc.BATCHES)
def test_every_batch_size_on_every_stream_count(ref, n):
    """Library defaults on the fast path (fused ReLU, aliases, first layer in place, host chunks of two panels from 512 images on),
    QCNN_OPT_STREAMS = 1 .. 4; then QCNN_OPT_KEEP_ALL = 1 once, every materialised map against the integer result."""
    eng = open_engine()
    seen = [check_forward(eng, ref, n, sc.config(streams=s)) for s in sc.STREAMS]
    seen.append(check_forward(eng, ref, n, sc.config(keep_all=1), every_map=True))
    print("%d images: streams 1-4, then KEEP_ALL = 1, ran %r: bit-equal to the integer result" % (n, seen))


# ---------------------------------------------------------------------------------------------- streams x host chunks
@pytest.mark.parametrize("keep_all", [0, 1])
@pytest.mark.parametrize("n", sc.CHUNK_BATCHES)
def test_streams_and_host_chunks(ref, n, keep_all):
    """QCNN_OPT_STREAMS 1 .. 4 x QCNN_OPT_HOST_CHUNK 0 .. 3 through qcnn_forward_host: chunks at pa > 0 writing into the whole-batch maps,
    unequal sub-batches (3 panels over 2 streams, 5 over 3 and 4, 9 over 4), a last chunk with fewer panels than streams."""
    eng = open_engine()
    seen = {(s, c): check_forward(eng, ref, n, sc.config(streams=s, chunk=c, keep_all=keep_all)) for s in sc.STREAMS for c in sc.CHUNKS}
    print("%d images, KEEP_ALL = %d: %d (streams, chunk) pairs, families %r" % (n, keep_all, len(seen), sorted(set(seen.values()))))


# ---------------------------------------------------------------------------------------------- the other options, one at a time
@pytest.mark.parametrize("opts", sc.OPTION_SETS, ids=lambda o: "-".join("%s%d" % kv for kv in sorted(o.items())))
def test_options_one_at_a_time(ref, opts):
    """QCNN_OPT_SPLIT = 0, the exact builder, QCNN_OPT_DEC_BF16SPLIT 0 / 1 (2 is the default), DIRECT_DEC, DECODE, SMALL_BATCH = 0,
    PACKED_FC = 1 at 3, 131, 385 and 1027 images, fast path and KEEP_ALL = 1."""
    eng = open_engine()
    for n in sc.OPTION_BATCHES:
        for keep in (0, 1):
            check_forward(eng, ref, n, sc.config(keep_all=keep, **opts))
    if "bf16split" in opts:
        assert eng.layer_dec_form(0)[0] == -1               # (KEEP_ALL = 1 ran last: the panel form)
        check_forward(eng, ref, 131, sc.config(**opts))
        form, pairs = eng.layer_dec_form(0)
        assert (form, pairs) == (opts.get("bf16split", 2), 0), (form, pairs)   # +-1 inputs are inside the fp16 form's range: no fix-up


# ---------------------------------------------------------------------------------------------- entry points
def test_device_input_and_host_batches(ref):
    """qcnn_forward (device pointers, enqueue only) and qcnn_forward_host_batches with the batch list 131, 3, 300, 1, 128, 640: the
    double-buffered schedule must route every batch's rows to its own arrays (each batch holds other images)."""
    import torch
    eng = open_engine()
    ensure_seen(eng, ref)
    dev = torch.device("cuda", 0)
    for keep in (0, 1):
        cfg = sc.config(keep_all=keep)
        set_cfg(eng, cfg)
        for n in sc.HOST_BATCH_LIST:
            idx = next_images(n)
            x = torch.from_numpy(np.ascontiguousarray(ref["x"][idx])).to(dev)
            prob = torch.empty((n, 10), dtype=torch.float32, device=dev)
            top5 = torch.empty((n, 5), dtype=torch.int16, device=dev)
            torch.cuda.synchronize(dev)
            eng.forward_dev(x.data_ptr(), n, prob.data_ptr(), top5.data_ptr())
            eng.sync()
            what = "qcnn_forward, %d images, KEEP_ALL = %d" % (n, keep)
            check_codes(eng, n, cfg, False, what)
            equal(eng.layer_output(sc.LAST_FC + 1, n), ref["want"][sc.LAST_FC + 1][idx], what)
            check_outputs(ref, idx, prob.cpu().numpy(), top5.cpu().numpy(), what)
        idxs = [next_images(n) for n in sc.HOST_BATCH_LIST]
        probs, top5s = eng.forward_host_batches([ref["x"][i] for i in idxs])
        what = "qcnn_forward_host_batches, KEEP_ALL = %d" % keep
        check_codes(eng, sc.HOST_BATCH_LIST[-1], cfg, False, what)
        equal(eng.layer_output(sc.LAST_FC + 1, sc.HOST_BATCH_LIST[-1]), ref["want"][sc.LAST_FC + 1][idxs[-1]], what)
        for b, (i, p, t) in enumerate(zip(idxs, probs, top5s)):
            assert _state["seen"][i].all()                 # (bit-equal to rows whose logits were held to the integer result)
            check_outputs(ref, i, p, t, "%s, batch %d" % (what, b))


# ---------------------------------------------------------------------------------------------- one engine, forward after forward
def test_forwards_back_to_back_and_option_toggles(ref):
    """1027 -> 3 -> 131 -> 1 -> 640 -> 1027 images enqueued on one engine with no synchronisation in between (qcnn_forward; every
    forward's probabilities must be the bits of rows whose logits were held to the integer result, the last one's logits are read
    back), then the same batch size before, under and after every option's other value: plan cache, lazily built tables, scratch."""
    import torch
    eng = open_engine()
    ensure_seen(eng, ref)
    dev = torch.device("cuda", 0)
    for keep in (0, 1):
        set_cfg(eng, sc.config(keep_all=keep))
        runs = []
        for n in sc.SEQUENCE:
            idx = next_images(n)
            runs.append((idx, torch.from_numpy(np.ascontiguousarray(ref["x"][idx])).to(dev),
                         torch.empty((n, 10), dtype=torch.float32, device=dev), torch.empty((n, 5), dtype=torch.int16, device=dev)))
        torch.cuda.synchronize(dev)
        for idx, x, prob, top5 in runs:
            eng.forward_dev(x.data_ptr(), len(idx), prob.data_ptr(), top5.data_ptr())
        eng.sync()
        equal(eng.layer_output(sc.LAST_FC + 1, N), ref["want"][sc.LAST_FC + 1][runs[-1][0]], "last forward of the sequence")
        for j, (idx, x, prob, top5) in enumerate(runs):
            assert _state["seen"][idx].all()
            check_outputs(ref, idx, prob.cpu().numpy(), top5.cpu().numpy(), "forward %d of the sequence (%d images), KEEP_ALL = %d" % (j, len(idx), keep))
    for n in (3, 385):
        for opts in sc.OPTION_SETS + (dict(streams=4), dict(chunk=1), dict(keep_all=1)):
            for cfg in (sc.config(), sc.config(**opts), sc.config()):
                check_forward(eng, ref, n, cfg)


# ---------------------------------------------------------------------------------------------- LRN
def test_lrn_table_across_the_fuse_gate():
    """conv -> ReLU -> LRN(5) -> pool 3x3 / 2 / 0 at 385 images (three full panels and one image): the conv / ReLU map is still the
    integer result; the pooled map lies inside glue_ref's interval around the float64 LRN of that integer map and has the same bits
    under every streams / chunk / KEEP_ALL setting (the fused kernel equals the separate ones bit for bit).  The gate
    qk_lrn_pool_blocks * (panels / ns) >= 192 is 64 * (panels / ns) here: open for the whole batch on one stream, shut on 2 .. 4
    streams and for chunks of one panel; the normalised map reported "not available" shows which way a forward went."""
    n = sc.LRN_N
    x, conv, relu = sc.lrn_reference()
    ly = sc.LRN_LAYERS[2]
    y64, s64 = gr.lrn64(relu, ly["siz"], ly["alp"], ly["bet"], ly["ini"])
    lo, mid, hi = gr.lrn_pool_interval(y64, gr.lrn_bound(y64, s64, ly["siz"], ly["bet"], False))
    eng = open_engine(sc.LRN_IN_CHW, sc.LRN_LAYERS, sc.lrn_params(), n)
    first, fused_seen = None, set()
    for keep in (0, 1):
        for s in sc.STREAMS:
            for c in (0, 1):
                what = "LRN table: streams %d, chunk %d, KEEP_ALL = %d" % (s, c, keep)
                set_cfg(eng, sc.config(streams=s, chunk=c, keep_all=keep))
                eng.forward_host(np.roll(x, 7, axis=0), want_prob=False, want_top5=False)      # other images in every buffer
                eng.forward_host(x, want_prob=False, want_top5=False)
                panels = [pb - pa for pa, pb in sc.chunks(n, c)]
                want_fused = not keep and any(sc.LRN_POOL_BLOCKS * (p // min(s, p)) >= sc.LRN_MIN_BLOCKS for p in panels)
                try:
                    eng.layer_output_range(3, 0, 1)
                    fused = False
                except RuntimeError:
                    fused = True
                assert fused == want_fused, what
                fused_seen.add(fused)
                if keep:
                    equal(eng.layer_output(1, n), conv.astype(np.float32), what + ": conv map")
                equal(eng.layer_output(2, n), relu.astype(np.float32), what + ": ReLU map")
                y = eng.layer_output(4, n)
                gr.check_interval(y, lo, mid, hi, what + ": pooled map")
                first = y if first is None else first
                assert np.array_equal(y.view(np.uint32), first.view(np.uint32)), what + ": pooled map differs from the first schedule's"
    assert fused_seen == {True, False}
    close_engine()
