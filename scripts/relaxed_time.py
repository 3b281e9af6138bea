#!/usr/bin/env python3
"""Device time of the Relaxed resize + pack and of the whole call (LABBOOK.md, "Relaxed resize on the device"):
qcnn_forward_u8_relaxed_views against qcnn_forward_u8_resized_views — the yardstick, unchanged code — at 1000 batch slots, 100
images x ten views and 1000 images x the centre view, from sources of 256 x 256 and of 500 x 375, nominal full size 256 x 256,
with a mean image (full-sized for the Strict call, crop-sized for the Relaxed one).

  pack step    a glue-only model ([relu]) of AlexNet's input shape, no output asked for: a call is the descriptor upload, the
               pack kernel and one ReLU sweep, HIP events around it; the differences between the variants are the pack step's.
  whole call   AlexNet with synthetic parameters, the fast path (QCNN_OPT_KEEP_ALL = 0), library defaults, prob + top-5 of the
               averaged rows.

Variants alternate inside one process after warm-up, every timed call behind an un-timed one of its kind (the host's
preparation of a call is then hidden behind device work); median, minimum and maximum.  Before anything is timed, the 256 x 256
sources (on which Relaxed is Strict) under the centre view must return the bits of qcnn_forward_u8_resized_views.
usage: relaxed_time.py [rounds=20]"""
import importlib, os, sys
import numpy as np
import torch   # before libqcnn_hip.so: both must bind to the HIP runtime torch ships
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n: importlib.import_module("quantized-cnn_amd." + n)

FULL = (256, 256)
SLOTS = 1000


def timed(stream, calls, rounds, warm=3):
    """{name: [ms]} of the calls, alternating, HIP events on the context's stream around each."""
    for _ in range(warm):
        for _, call in calls:
            call()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in calls}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(rounds):
        for name, call in calls:
            call()                 # un-timed: keeps the device busy while the host prepares the timed call behind it
            ev[0].record(stream)
            call()
            ev[1].record(stream)
            ev[1].synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    return ms


def report(title, ms):
    """Every relaxed variant against the resized call on the same sources and slot split (the line before it)."""
    print(title)
    base = None
    for name, v in ms.items():
        med = float(np.median(v))
        if name.startswith("u8_resized"):
            base = med
        print("  %-58s median %.3f ms  min %.3f ms  max %.3f ms  x %.3f of the resized call" % (name, med, min(v), max(v), med / base))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    capi, topo, synth, engine = pkg("capi"), pkg("topology"), pkg("synth"), pkg("engine")
    in_chw, layers, _, _ = topo.MODELS["AlexNet"]
    c, h, w = in_chw
    rng = np.random.default_rng(9)
    full_mean = (rng.standard_normal((c,) + FULL) * 20 + 110).astype(np.float32)
    ten = engine.ten_crop_views(FULL[0], FULL[1], h, w)
    centre = [ten[4]]
    oy, ox, _ = ten[4]
    mean = torch.from_numpy(full_mean).cuda()
    mean_crop = torch.from_numpy(np.ascontiguousarray(full_mean[:, oy:oy + h, ox:ox + w])).cuda()    # the centre view's window
    ten_a, centre_a = engine.ten_crop_anchored(), [(1, 1, 0, 0, 0)]
    sources = {}
    for hs, ws in ((256, 256), (500, 375)):
        px = torch.from_numpy(rng.integers(0, 256, (SLOTS, c, hs, ws), dtype=np.uint8)).cuda()
        descs = {n: (capi.QcnnSrcImage * n)(*[capi.QcnnSrcImage(i * c * hs * ws, hs, ws) for i in range(n)]) for n in (SLOTS // 10, SLOTS)}
        sources[(hs, ws)] = (px, descs)
        print("source %dx%d: relaxed full size %dx%d, scale %r" % ((hs, ws) + engine.relaxed_full_size(hs, ws, *FULL)))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def variants(eng, outs):
        """[(name, call)]: per slot split and source size the resized call, then the relaxed one."""
        calls = []
        for n, views, aviews, label in ((SLOTS // 10, ten, ten_a, "%d images x ten views" % (SLOTS // 10)), (SLOTS, centre, centre_a, "%d images x centre" % SLOTS)):
            for (hs, ws), (px, descs) in sources.items():
                calls.append(("u8_resized_views  %dx%d  %s" % (hs, ws, label),
                              lambda n=n, views=views, px=px, descs=descs: eng.forward_u8_resized_views_dev(
                                  px.data_ptr(), px.numel(), descs[n], FULL[0], FULL[1], mean.data_ptr(), views, *outs)))
                calls.append(("u8_relaxed_views  %dx%d  %s" % (hs, ws, label),
                              lambda n=n, aviews=aviews, px=px, descs=descs: eng.forward_u8_relaxed_views_dev(
                                  px.data_ptr(), px.numel(), descs[n], FULL[0], FULL[1], mean_crop.data_ptr(), aviews, *outs)))
        return calls

    # ---- the pack step: glue-only model, no outputs
    glue = engine.QcnnEngine(0, stream=stream.cuda_stream)
    glue.set_option(capi.OPT_KEEP_ALL, 1)
    glue.load_model(in_chw, [topo.relu()], {}, SLOTS)
    calls = variants(glue, (None, None, None))
    assert "256x256" in calls[4][0] and "centre" in calls[4][0] and "resized" in calls[4][0] and "relaxed" in calls[5][0]
    calls[4][1]()
    glue.sync()
    want = glue.layer_output_range(0, 0, 16)
    calls[5][1]()
    glue.sync()
    same = np.array_equal(want.view(np.uint32), glue.layer_output_range(0, 0, 16).view(np.uint32))
    print("fm[0] of 256x256 sources, centre view, Relaxed against Strict (16 slots): %s" % ("same bits" if same else "DIFFERENT"))
    if not same:
        sys.exit(1)
    report("pack kernel + one ReLU sweep over %d x %d floats (glue-only model):" % (SLOTS, c * h * w), timed(stream, calls, rounds))
    glue.close()

    # ---- the whole call: AlexNet
    eng = engine.QcnnEngine(0, stream=stream.cuda_stream)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.load_model(in_chw, layers, synth.make_params(in_chw, layers, seed=0), SLOTS)
    prob = torch.empty((SLOTS, 1000), dtype=torch.float32, device="cuda")
    top5 = torch.empty((SLOTS, 5), dtype=torch.int16, device="cuda")
    prob_r, top5_r = torch.empty_like(prob), torch.empty_like(top5)
    calls = variants(eng, (prob.data_ptr(), top5.data_ptr(), None))
    check = variants(eng, (prob_r.data_ptr(), top5_r.data_ptr(), None))
    calls[4][1]()
    check[5][1]()
    eng.sync()
    same = bool(torch.equal(prob.view(torch.int32), prob_r.view(torch.int32)) and torch.equal(top5, top5_r))
    print("AlexNet, 256x256 sources, centre view, Relaxed against Strict (1000 images): %s" % ("same bits" if same else "DIFFERENT"))
    if not same:
        sys.exit(1)
    report("whole call, AlexNet (prob + top-5 of the averaged rows):", timed(stream, calls, rounds))
    eng.close()


if __name__ == "__main__":
    main()
