#!/usr/bin/env python3
"""Whole-call device time of multi-view inference against the single-view 8-bit forward (LABBOOK.md, "Multi-view inference"):
qcnn_forward_u8_views on 100 images x ten-crop (1000 batch slots) and qcnn_forward_u8 on 1000 images, AlexNet with synthetic
parameters, 256 x 256 sources with a mean image, the fast path (QCNN_OPT_KEEP_ALL = 0), otherwise the library's defaults.  HIP
events on the context's stream around each call, the two calls alternating, after warm-up; median and minimum.  Before anything
is timed, 1000 images under the single centre view must return the bits of qcnn_forward_u8.
usage: views_time.py [rounds=20]"""
import importlib, os, sys
import numpy as np
import torch   # before libqcnn_hip.so: both must bind to the HIP runtime torch ships
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n: importlib.import_module("quantized-cnn_amd." + n)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    capi, topo, synth, engine = pkg("capi"), pkg("topology"), pkg("synth"), pkg("engine")
    in_chw, layers, _, _ = topo.MODELS["AlexNet"]
    c, h, w = in_chw
    hs = ws = 256
    n1, n10 = 1000, 100
    stream = torch.cuda.Stream()
    eng = engine.QcnnEngine(0, stream=stream.cuda_stream)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.load_model(in_chw, layers, synth.make_params(in_chw, layers, seed=0), n1)
    rng = np.random.default_rng(9)
    px = torch.from_numpy(rng.integers(0, 256, (n1, c, hs, ws), dtype=np.uint8)).cuda()
    mean = torch.from_numpy((rng.standard_normal((c, hs, ws)) * 20 + 110).astype(np.float32)).cuda()
    views = engine.ten_crop_views(hs, ws, h, w)
    prob = torch.empty((n1, 1000), dtype=torch.float32, device="cuda")
    top5 = torch.empty((n1, 5), dtype=torch.int16, device="cuda")
    prob_v = torch.empty((n1, 1000), dtype=torch.float32, device="cuda")
    top5_v = torch.empty((n1, 5), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()

    def single():
        eng.forward_u8_dev(px.data_ptr(), hs, ws, mean.data_ptr(), n1, prob.data_ptr(), top5.data_ptr())

    def multi():
        eng.forward_u8_views_dev(px.data_ptr(), hs, ws, mean.data_ptr(), n10, views, prob_v.data_ptr(), top5_v.data_ptr())

    single()
    eng.forward_u8_views_dev(px.data_ptr(), hs, ws, mean.data_ptr(), n1, [views[4]], prob_v.data_ptr(), top5_v.data_ptr())
    eng.sync()
    same = bool(torch.equal(prob.view(torch.int32), prob_v.view(torch.int32)) and torch.equal(top5, top5_v))
    print("1000 images under the centre view against qcnn_forward_u8: %s" % ("same bits" if same else "DIFFERENT"))
    if not same:
        sys.exit(1)
    for _ in range(3):
        single()
        multi()
    eng.sync()
    ms = {"single": [], "multi": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(rounds):
        for name, call in (("single", single), ("multi", multi)):
            ev[0].record(stream)
            call()
            ev[1].record(stream)
            ev[1].synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print("qcnn_forward_u8        1000 images             median %.3f ms  min %.3f ms  max %.3f ms" % (med["single"], min(ms["single"]), max(ms["single"])))
    print("qcnn_forward_u8_views  100 images x ten-crop   median %.3f ms  min %.3f ms  max %.3f ms  x %.3f of qcnn_forward_u8"
          % (med["multi"], min(ms["multi"]), max(ms["multi"]), med["multi"] / med["single"]))
    eng.close()


if __name__ == "__main__":
    main()
