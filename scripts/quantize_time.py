"""Time the dense -> Q-CNN quantiser (QcnnEngine.quantize_layer, qcnn_quantize_layer) per layer on synthetic dense weights
at the shipped layout rule (synth.quant_spec), against the numpy restatement of its contract (tests/pq_oracle.py).

    python scripts/quantize_time.py [--models AlexNet VGG16] [--max-iter 30] [--oracle-models AlexNet]
    python scripts/quantize_time.py --kernel-stats DIR     # summarise a rocprofv3 --kernel-trace --stats run of the above

One JSON line per model: per conv / FC layer the wall time of one call after a warm-up call (host -> device copy of the
weights, kernels, device -> host copies of the results), update steps taken, sub-spaces still changing at max_iter, and the
numpy oracle's wall time for the same call (and whether its bytes match) where requested.  Kernel times come from a separate
rocprofv3 run (tracing slows the host): --kernel-stats prints its k_pq_* rows as one JSON line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["AlexNet", "VGG16"])
    ap.add_argument("--max-iter", type=int, default=None)
    ap.add_argument("--oracle-models", nargs="*", default=["AlexNet"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats)
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
