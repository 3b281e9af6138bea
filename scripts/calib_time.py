"""Time the resident calibration (qcnn_calib_begin .. qcnn_calib_read, kernel k_ec_gram_panel) on AlexNet with synthetic dense
weights (synth.make_dense_params, as scripts/quantize_time.py makes them).

    python scripts/calib_time.py [--slots 1000] [--batches 3] [--images 256] [--chunk 32] [--repeats 3]

One JSON line:
  (a) stream: ms per --slots-slot batch of forward_u8_host_batches on the dense model (planar 256 x 256 sources, centre view),
      unarmed, and armed with all eight conv / FC layers listed — median of --repeats calls of --batches batches after a
      warm-up call; the difference is what the gram launches cost.
  (b) calibrate: seconds per image of quantize.calibrate as it always was (every map to the host and back, chunk --chunk,
      --images images), of calibrate(resident=True) and of calibrate_u8 on the same pixels.  Each figure is the wall time of the
      whole call — model load, forwards, the download of the eight matrices — after a warm-up call on one chunk, divided by
      the images; max_rel_diff compares the resident matrices with the host-path ones.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pkg(name):
    return importlib.import_module("quantized-cnn_amd." + name)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1000)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    topo, synth, engine, quantize, capi = pkg("topology"), pkg("synth"), pkg("engine"), pkg("quantize"), pkg("capi")
    in_chw, layers = topo.MODELS["AlexNet"][:2]
    dense = synth.make_dense_params(in_chw, layers, seed=a.seed)
    ids = sorted(dense)
    rng = np.random.default_rng(a.seed + 1)
    out = dict(model="AlexNet", layers=ids)

    # (a) the stream, unarmed and armed
    full = (256, 256)
    srcs = [rng.integers(0, 256, (in_chw[0],) + full).astype(np.uint8) for _ in range(a.slots)]
    flat, descs, _ = engine.split_batches(srcs, None, a.slots, 1)[0]
    pin = engine.host_alloc(flat.size)
    pin[:] = flat
    batches = [(pin, descs)] * a.batches
    eng = engine.QcnnEngine(0)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.load_dense_model(in_chw, layers, dense, a.slots)

    def stream_ms():
        eng.forward_u8_host_batches(batches, full, want=(False, True, False))          # warm-up
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            eng.forward_u8_host_batches(batches, full, want=(False, True, False))
            ms.append((time.perf_counter() - t0) * 1e3 / a.batches)
        return round(median(ms), 3), [round(min(ms), 3), round(max(ms), 3)]

    unarmed = stream_ms()
    eng.calib_begin(ids)
    armed = stream_ms()
    rows = {i: eng.calib_read(i)[1] for i in ids}
    eng.calib_end()
    eng.close()
    engine.host_free(pin)
    out["stream"] = dict(slots=a.slots, batches=a.batches, unarmed_ms_per_batch=unarmed[0], unarmed_min_max=unarmed[1],
                         armed_ms_per_batch=armed[0], armed_min_max=armed[1], rows_added={str(i): int(r) for i, r in rows.items()})
    print("# stream: %s" % out["stream"], file=sys.stderr, flush=True)

    # (b) calibrate as it was, resident, and from 8-bit sources
    u8 = [rng.integers(0, 256, tuple(in_chw)).astype(np.uint8) for _ in range(a.images)]
    imgs = np.stack(u8).astype(np.float32)
    cut = engine.split_batches(u8, None, a.images, 1)
    hw = (in_chw[1], in_chw[2])
    eng = engine.QcnnEngine(0)
    paths = dict(
        host=lambda x, c: quantize.calibrate(eng, in_chw, layers, dense, x, chunk=a.chunk),
        resident=lambda x, c: quantize.calibrate(eng, in_chw, layers, dense, x, chunk=a.chunk, resident=True),
        u8=lambda x, c: quantize.calibrate_u8(eng, in_chw, layers, dense, c, hw))
    warm = engine.split_batches(u8[:a.chunk], None, a.chunk, 1)
    res, secs = {}, {}
    for name, call in paths.items():
        call(imgs[:a.chunk], warm)                                                     # warm-up on one chunk
        t0 = time.perf_counter()
        res[name] = call(imgs, cut)
        secs[name] = time.perf_counter() - t0
        print("# calibrate %s: %.3f s for %d images" % (name, secs[name], a.images), file=sys.stderr, flush=True)
    eng.close()
    diff = lambda x, y: max(float(np.abs(x[i] - y[i]).max() / max(np.abs(y[i]).max(), 1e-300)) for i in ids)
    out["calibrate"] = dict(images=a.images, chunk=a.chunk,
                            host_s_per_image=round(secs["host"] / a.images, 5),
                            resident_s_per_image=round(secs["resident"] / a.images, 5),
                            u8_s_per_image=round(secs["u8"] / a.images, 5),
                            host_over_resident=round(secs["host"] / secs["resident"], 2),
                            resident_vs_host_max_rel_diff=diff(res["resident"], res["host"]),
                            u8_vs_host_max_rel_diff=diff(res["u8"], res["host"]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
