#!/usr/bin/env python3
"""Wall time per batch of 8-bit source batches streamed from host memory (LABBOOK.md, "Streaming 8-bit sources"):
qcnn_forward_u8_resized_host_batches against what a caller had before it.  AlexNet with synthetic parameters, the fast path
(QCNN_OPT_KEEP_ALL = 0), full image 256 x 256 with a mean image; BATCHES batches of 1000 batch slots each, as 1000 images x the
centre view and as 100 images x ten-crop, planar sources of 256 x 256 and of 500 x 375 in qcnn_host_alloc memory (two source
buffers, the batches alternating between them, as the two float buffers of (4) do).

  (1) stream            the new call, prob + top-5 asked for, no labels
  (2) blocking loop     forward_u8_resized_host batch after batch: upload, run, sync, download, nothing overlapped
  (3) device-resident   forward_u8_resized_views_strided_dev on the same batches, sources uploaded beforehand: the floor
  (4) float pipeline    forward_host_batches on 1000 float crops (3 x 227 x 227) a batch from pinned memory: the yardstick
  (5) stream + labels   (1) with a label per image: against (1), the cost of counting

Every call is blocking or ends in a synchronise; the clock is the host's around the whole call, divided by the batches.  After one
warm-up of each, REPS repetitions with the five alternating; median, minimum - maximum.  Before anything is timed batch 0 of (1)
must have the bits of (3).
usage: stream_time.py [batches=8] [reps=5] [--schedule]
  --schedule   instead of timing: QCNN_DEBUG_PIPELINE=1 and one call of (1) per shape, the schedule on stderr"""
import importlib, os, sys, time
if "--schedule" in sys.argv:
    os.environ["QCNN_DEBUG_PIPELINE"] = "1"           # read once, when the library first streams
import numpy as np
import torch   # before libqcnn_hip.so: both must bind to the HIP runtime torch ships
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n: importlib.import_module("quantized-cnn_amd." + n)

FULL = (256, 256)
SLOTS = 1000
SIZES = ((256, 256), (500, 375))


def pinned_copy(engine, a):
    flat = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    p = engine.host_alloc(flat.size)
    p[:] = flat
    return p


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    nb = int(args[0]) if args else 8
    reps = int(args[1]) if len(args) > 1 else 5
    schedule = "--schedule" in sys.argv
    capi, topo, synth, engine = pkg("capi"), pkg("topology"), pkg("synth"), pkg("engine")
    in_chw, layers, _, _ = topo.MODELS["AlexNet"]
    c, h, w = in_chw
    rng = np.random.default_rng(9)
    mean = (rng.standard_normal((c,) + FULL) * 20 + 110).astype(np.float32)
    d_mean = torch.from_numpy(mean).cuda()
    ten = engine.ten_crop_views(FULL[0], FULL[1], h, w)
    stream = torch.cuda.Stream()
    eng = engine.QcnnEngine(0, stream=stream.cuda_stream)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.load_model(in_chw, layers, synth.make_params(in_chw, layers, seed=0), SLOTS)
    # (4): two pinned float batches, alternating
    crops = [pinned_copy(engine, rng.standard_normal((SLOTS, c, h, w), dtype=np.float32) * 50).view(np.float32).reshape(SLOTS, c, h, w)
             for _ in range(2)]
    floats = [crops[b & 1] for b in range(nb)]
    d_prob = torch.empty((SLOTS, 1000), dtype=torch.float32, device="cuda")
    d_top5 = torch.empty((SLOTS, 5), dtype=torch.int16, device="cuda")
    labels_all = rng.integers(0, 1000, SLOTS).astype(np.uint16)
    print("AlexNet, %d batches of %d slots a call, %d repetitions; ms PER BATCH: median (min - max)" % (nb, SLOTS, reps))
    for n, views, shape in ((SLOTS, [ten[4]], "%d x centre" % SLOTS), (SLOTS // 10, ten, "%d x ten-crop" % (SLOTS // 10))):
        for hs, ws in SIZES:
            src = [pinned_copy(engine, rng.integers(0, 256, (n, c, hs, ws), dtype=np.uint8)) for _ in range(2)]
            desc_list = [engine.src_planar(i * c * hs * ws, hs, ws, c) for i in range(n)]
            descs = engine._pixels_array(desc_list)[0]                # made once: no per-call conversion in (1), (3), (5)
            batches = [(src[b & 1], descs) for b in range(nb)]
            outs = [(np.empty((n, 1000), np.float32), np.empty((n, 5), np.uint16), None) for _ in range(nb)]
            labels = [labels_all[:n]] * nb
            hits = np.zeros(5, np.uint64)
            d_src = [torch.from_numpy(s).cuda() for s in src]
            torch.cuda.synchronize()

            def stream_call(lab=None):
                eng.forward_u8_host_batches_into(batches, FULL, d_mean.data_ptr(), views, "strict", outs, lab, hits if lab is not None else None)

            def blocking_loop():
                for flat, _ in batches:
                    eng.forward_u8_resized_host(None, FULL, mean, views, descs=(flat, desc_list))

            def resident():
                for b in range(nb):
                    eng.forward_u8_resized_views_strided_dev(d_src[b & 1].data_ptr(), src[b & 1].size, descs, FULL[0], FULL[1], d_mean.data_ptr(),
                                                             views, d_prob.data_ptr(), d_top5.data_ptr())
                eng.sync()

            tag = "%dx%d  %s  (%.1f MB of source bytes a batch, %.1f MB of float crops)" % (hs, ws, shape, src[0].size / 1e6, crops[0].nbytes / 1e6)
            if schedule:
                print(tag, file=sys.stderr)
                stream_call()
            else:
                stream_call()
                resident()
                eng.forward_u8_resized_views_strided_dev(d_src[0].data_ptr(), src[0].size, descs, FULL[0], FULL[1], d_mean.data_ptr(), views,
                                                         d_prob.data_ptr(), d_top5.data_ptr())
                eng.sync()
                first = (d_prob[:n].cpu().numpy(), d_top5[:n].cpu().numpy().view(np.uint16))
                same = np.array_equal(first[0].view(np.uint32), outs[0][0].view(np.uint32)) and np.array_equal(first[1], outs[0][1])
                print(tag)
                print("  batch 0 of (1) against (3): %s" % ("same bits" if same else "DIFFERENT"))
                if not same:
                    sys.exit(1)
                calls = (("(1) stream", stream_call), ("(2) blocking loop", blocking_loop), ("(3) device-resident", resident),
                         ("(4) float pipeline", lambda: eng.forward_host_batches(floats)), ("(5) stream + labels", lambda: stream_call(labels)))
                for _, call in calls:
                    call()
                ms = {name: [] for name, _ in calls}
                for _ in range(reps):
                    for name, call in calls:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        call()
                        ms[name].append((time.perf_counter() - t0) * 1e3 / nb)
                med = {k: float(np.median(v)) for k, v in ms.items()}
                for name, v in ms.items():
                    print("  %-20s %8.3f (%.3f - %.3f)" % (name, med[name], min(v), max(v)))
                lo, hi = min(ms["(4) float pipeline"]), max(ms["(4) float pipeline"])
                print("  (1) / (4) = %.3f   [(4) itself spreads %.3f - %.3f of its median]   (1) / (3) = %.3f   (5) / (1) = %.3f   (2) / (1) = %.3f"
                      % (med["(1) stream"] / med["(4) float pipeline"], lo / med["(4) float pipeline"], hi / med["(4) float pipeline"],
                         med["(1) stream"] / med["(3) device-resident"], med["(5) stream + labels"] / med["(1) stream"],
                         med["(2) blocking loop"] / med["(1) stream"]))
            del d_src
            for s in src:
                engine.host_free(s)
    for a in crops:
        engine.host_free(a.reshape(-1).view(np.uint8))
    eng.close()


if __name__ == "__main__":
    main()
