"""Time the dense -> Q-CNN quantiser (QcnnEngine.quantize_layer, qcnn_quantize_layer) per layer on synthetic dense weights
at the shipped layout rule (synth.quant_spec), against the numpy restatement of its contract (tests/pq_oracle.py).

    python scripts/quantize_time.py [--models AlexNet VGG16] [--max-iter 30] [--oracle-models AlexNet]
    python scripts/quantize_time.py --kernel-stats DIR     # summarise a rocprofv3 --kernel-trace --stats run of the above
    python scripts/quantize_time.py --ec [--ec-images 64] [--ec-sweep]   # error-corrected quantisation, per layer of --models

One JSON line per model: per conv / FC layer the wall time of one call after a warm-up call (host -> device copy of the
weights, kernels, device -> host copies of the results), update steps taken, sub-spaces still changing at max_iter, and the
numpy oracle's wall time for the same call (and whether its bytes match) where requested.  Kernel times come from a separate
rocprofv3 run (tracing slows the host): --kernel-stats prints its k_pq_* rows as one JSON line.

--ec: per conv / FC layer the wall time of QcnnEngine.calib_gram (qcnn_calib_gram: upload, k_ec_gram, download of the fp64
matrix) on synthetic post-ReLU input maps of --ec-images images (median of --ec-repeats calls after a warm-up call), beside numpy's ``X.T @ X`` on the
float32 patch matrix of the same input on the host of the same box (its im2col is not timed), and with --ec-sweep the wall
time of ONE sweep of quantize_layer_ec from the k-means start (copies and the two fp64 evaluations of J included).
"""
from __future__ import annotations

import argparse
import csv
import glob
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pkg(name):
    return importlib.import_module("quantized-cnn_amd." + name)


def kernel_stats(dir_path):
    files = glob.glob(os.path.join(dir_path, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % dir_path)
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if "k_pq_" in r.get("Name", ""):
                    rows.append(dict(name=r["Name"], calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) / 1e6,
                                     avg_us=float(r["AverageNs"]) / 1e3))
    rows.sort(key=lambda r: -r["total_ms"])
    print(json.dumps(dict(kernel_stats=rows, total_ms=round(sum(r["total_ms"] for r in rows), 3))))


def ec_times(a):
    import numpy as np
    import ec_oracle
    topo, synth, engine, quantize = pkg("topology"), pkg("synth"), pkg("engine"), pkg("quantize")
    eng = engine.QcnnEngine(0)
    for model in a.models:
        in_chw, layers = topo.MODELS[model][:2]
        sizes = topo.fmap_sizes(in_chw, layers)
        dense = synth.make_dense_params(in_chw, layers, seed=a.seed)
        spec = synth.quant_spec(in_chw, layers)
        rows = []
        for i in sorted(dense):
            h, w_, c = sizes[i]
            g = quantize.layer_geom(layers, i)
            shape = (a.ec_images, h, w_, c) if g["kh"] > 1 or layers[i]["type"] == topo.CONV else (a.ec_images, 1, 1, h * w_ * c)
            x = np.maximum(np.random.default_rng(a.seed + i).standard_normal(shape), 0).astype(np.float32)
            eng.calib_gram(x, g)                                                       # warm-up
            walls = []
            for _ in range(a.ec_repeats):
                t0 = time.perf_counter()
                G = eng.calib_gram(x, g)
                walls.append(time.perf_counter() - t0)
            wall = sorted(walls)[len(walls) // 2]
            X = ec_oracle.patches(x, g["grp"], g["kh"], g["kw"], g["stride"], g["pad"]).astype(np.float32)
            t0 = time.perf_counter()
            ref = np.stack([m.T @ m for m in X])
            np_s = time.perf_counter() - t0
            row = dict(layer=i, grp=g["grp"], P=int(G.shape[1]), rows=int(X.shape[1]), gram_ms=round(wall * 1e3, 3), gram_ms_min_max=[round(min(walls) * 1e3, 3), round(max(walls) * 1e3, 3)], numpy_ms=round(np_s * 1e3, 3),
                       max_rel_diff=float(np.abs(G - ref).max() / max(np.abs(ref).max(), 1e-30)))
            if a.ec_sweep:
                s, wt = spec[i], np.ascontiguousarray(dense[i]["weights"])
                ctrd, asmt, _ = eng.quantize_layer(wt, s["M"], s["K"], s["Cs"], max_iter=10)
                t0 = time.perf_counter()
                _, _, st = eng.quantize_layer_ec(wt, s["M"], s["K"], s["Cs"], G, ctrd, asmt, grp=g["grp"], sweeps=1)
                row.update(sweep_ms=round((time.perf_counter() - t0) * 1e3, 1), obj_init=st["obj_init"], obj=st["obj"],
                           changed=int(st["changed"][0]))
            rows.append(row)
            print("# %s layer %d: %s" % (model, i, row), file=sys.stderr, flush=True)
        print(json.dumps(dict(model=model, ec_images=a.ec_images, layers=rows)), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["AlexNet", "VGG16"])
    ap.add_argument("--max-iter", type=int, default=None)
    ap.add_argument("--oracle-models", nargs="*", default=["AlexNet"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--ec", action="store_true")
    ap.add_argument("--ec-images", type=int, default=64)
    ap.add_argument("--ec-sweep", action="store_true")
    ap.add_argument("--ec-repeats", type=int, default=5)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats)
    if a.ec:
        return ec_times(a)
    import numpy as np
    import pq_oracle
    topo, synth, engine = pkg("topology"), pkg("synth"), pkg("engine")
    max_iter = engine.DEFAULT_MAX_ITER if a.max_iter is None else a.max_iter
    eng = engine.QcnnEngine(0)
    for model in a.models:
        in_chw, layers = topo.MODELS[model][:2]
        dense = synth.make_dense_params(in_chw, layers, seed=a.seed)
        spec = synth.quant_spec(in_chw, layers)
        rows = []
        for i in sorted(dense):
            s, w = spec[i], np.ascontiguousarray(dense[i]["weights"])
            eng.quantize_layer(w, s["M"], s["K"], s["Cs"], max_iter=max_iter)           # warm-up
            t0 = time.perf_counter()
            ctrd, asmt, st = eng.quantize_layer(w, s["M"], s["K"], s["Cs"], max_iter=max_iter)
            wall = time.perf_counter() - t0
            row = dict(layer=i, kind=s["kind"], M=s["M"], K=s["K"], Cs=s["Cs"], N=int(w.size // w.shape[1]),
                       weight_mb=round(w.nbytes / 2 ** 20, 1), wall_ms=round(wall * 1e3, 3), iters=st["iters"],
                       unconverged=st["unconverged"], sse_init=st["sse_init"], sse=st["sse"])
            if model in (a.oracle_models or []):
                t0 = time.perf_counter()
                oc, oa, ost = pq_oracle.quantize_layer(w, s["M"], s["K"], s["Cs"], max_iter=max_iter)
                row["oracle_s"] = round(time.perf_counter() - t0, 3)
                row["oracle_match"] = bool(oc.tobytes() == ctrd.tobytes() and oa.tobytes() == asmt.tobytes()
                                           and (ost["iters"], ost["unconverged"]) == (st["iters"], st["unconverged"]))
            rows.append(row)
            print("# %s layer %d: %s" % (model, i, row), file=sys.stderr, flush=True)
        out = dict(model=model, max_iter=max_iter, layers=rows, total_wall_ms=round(sum(r["wall_ms"] for r in rows), 3))
        if all("oracle_s" in r for r in rows):
            out["total_oracle_s"] = round(sum(r["oracle_s"] for r in rows), 3)
        print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
