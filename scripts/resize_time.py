#!/usr/bin/env python3
"""Device time of the fused resize + pack and of the whole call (LABBOOK.md, "Resize on the device"): qcnn_forward_u8_resized_views
against qcnn_forward_u8_views at 1000 batch slots — 100 images x ten-crop and 1000 images x the centre view — from sources of
256 x 256 (the full size: what qcnn_forward_u8_views needs) and of 500 x 375, full image 256 x 256 with a mean image.

  pack step    a glue-only model ([relu]) of AlexNet's input shape, no output asked for: a call is the descriptor upload, the
               pack kernel and one ReLU sweep, HIP events around it; the differences between the variants are the pack step's
               (k_pack_u8_views is the yardstick; the kernels alone: scripts/ubench/pack_resized.hip).
  whole call   AlexNet with synthetic parameters, the fast path (QCNN_OPT_KEEP_ALL = 0), library defaults, prob + top-5 of the
               averaged rows; conv1's launch at the same batch from QCNN_OPT_PROFILE for comparison.

Variants alternate inside one process after warm-up, every timed call behind an un-timed one of its kind (the host's
preparation of a call is then hidden behind device work); median, minimum and maximum.  Before anything is timed, full-size sources
must return the bits of qcnn_forward_u8_views.
usage: resize_time.py [rounds=20]"""
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


def report(title, ms, yardstick):
    print(title)
    base = float(np.median(ms[yardstick]))
    for name, v in ms.items():
        print("  %-58s median %.3f ms  min %.3f ms  max %.3f ms  x %.3f of %s" % (name, float(np.median(v)), min(v), max(v), float(np.median(v)) / base, yardstick))
    return {name: float(np.median(v)) for name, v in ms.items()}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    capi, topo, synth, engine = pkg("capi"), pkg("topology"), pkg("synth"), pkg("engine")
    in_chw, layers, _, _ = topo.MODELS["AlexNet"]
    c, h, w = in_chw
    rng = np.random.default_rng(9)
    mean = torch.from_numpy((rng.standard_normal((c,) + FULL) * 20 + 110).astype(np.float32)).cuda()
    ten = engine.ten_crop_views(FULL[0], FULL[1], h, w)
    centre = [ten[4]]
    sources = {}
    for hs, ws in ((256, 256), (500, 375)):
        px = torch.from_numpy(rng.integers(0, 256, (SLOTS, c, hs, ws), dtype=np.uint8)).cuda()
        # what engine.pack_sources gives for equal sizes, as ready ctypes arrays of 100 and of 1000 descriptors
        descs = {n: (capi.QcnnSrcImage * n)(*[capi.QcnnSrcImage(i * c * hs * ws, hs, ws) for i in range(n)]) for n in (SLOTS // 10, SLOTS)}
        sources[(hs, ws)] = (px, descs)
    px256 = sources[(256, 256)][0]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def variants(eng, outs):
        """[(name, call)]: the views call on 256 x 256 sources, then the resized call on both source sizes, per slot split."""
        calls = []
        for n, views, label in ((SLOTS // 10, ten, "%d images x ten-crop" % (SLOTS // 10)), (SLOTS, centre, "%d images x centre" % SLOTS)):
            calls.append(("u8_views          256x256  " + label,
                          lambda n=n, views=views: eng.forward_u8_views_dev(px256.data_ptr(), FULL[0], FULL[1], mean.data_ptr(), n, views, *outs)))
            for (hs, ws), (px, descs) in sources.items():
                calls.append(("u8_resized_views  %dx%d  %s" % (hs, ws, label),
                              lambda n=n, views=views, px=px, descs=descs: eng.forward_u8_resized_views_dev(
                                  px.data_ptr(), px.numel(), descs[n], FULL[0], FULL[1], mean.data_ptr(), views, *outs)))
        return calls

    # ---- the pack step: glue-only model, no outputs
    glue = engine.QcnnEngine(0, stream=stream.cuda_stream)
    glue.set_option(capi.OPT_KEEP_ALL, 1)
    glue.load_model(in_chw, [topo.relu()], {}, SLOTS)
    calls = variants(glue, (None, None, None))
    calls[0][1]()
    glue.sync()
    want = glue.layer_output_range(0, 0, 16)
    calls[1][1]()
    glue.sync()
    same = np.array_equal(want.view(np.uint32), glue.layer_output_range(0, 0, 16).view(np.uint32))
    print("fm[0] of full-size sources through the resize against qcnn_forward_u8_views (16 slots): %s" % ("same bits" if same else "DIFFERENT"))
    if not same:
        sys.exit(1)
    report("pack kernel + one ReLU sweep over %d x %d floats (glue-only model):" % (SLOTS, c * h * w), timed(stream, calls, rounds), calls[0][0])
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
    calls[0][1]()
    check[1][1]()
    eng.sync()
    same = bool(torch.equal(prob[:SLOTS // 10].view(torch.int32), prob_r[:SLOTS // 10].view(torch.int32)) and torch.equal(top5[:SLOTS // 10], top5_r[:SLOTS // 10]))
    print("AlexNet, full-size sources through the resize against qcnn_forward_u8_views (100 images x ten-crop): %s" % ("same bits" if same else "DIFFERENT"))
    if not same:
        sys.exit(1)
    report("whole call, AlexNet (prob + top-5 of the averaged rows):", timed(stream, calls, rounds), calls[0][0])
    eng.set_option(capi.OPT_PROFILE, 1)
    for _ in range(rounds):
        calls[0][1]()
    eng.sync()
    tot, _, fw = eng.layer_total_ms()
    print("  conv1 at %d slots (QCNN_OPT_PROFILE, mean of %d): %.3f ms" % (SLOTS, fw, float(tot[0]) / max(fw, 1)))
    eng.close()


if __name__ == "__main__":
    main()
