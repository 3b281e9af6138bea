"""Propagated response error of a quantised AlexNet against the dense one, on the device (quantize.response_report,
qcnn_map_diff), with synthetic weights and inputs (synth.make_dense_params, synth.quant_spec, synth.make_images) — the figures
show the instrument working, they are not ImageNet accuracy.

    python scripts/response_report.py [--batch 1000] [--calib 256] [--sweeps 1] [--repeats 3] [--seed 0]

The dense model sits in one engine; a second one holds the k-means quantisation, then the error-corrected one
(quantize.calibrate(resident=True) on --calib images of another seed, quantize_model(calib=...)).  Printed per conv / FC layer:
the weight rel_err |W - W_hat| / |W|, the EC objective before -> after, the propagated rel_err of the layer's output map under
both quantisations, then `agree` of both.  Two times for one --batch-image batch whose maps both engines hold: the device report
over all default maps (median of --repeats after a warm-up call), and the host route it replaces — layer_output of both engines
plus the same sums in numpy float64 — once.  One JSON line at the end.
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


def host_route(np, eng, ref, maps, n, step=50):
    """What the device call replaces: both maps to the host, the six sums in numpy float64 (images in steps, to bound memory)."""
    out = {}
    for l in maps:
        a, b = eng.layer_output(l, n), ref.layer_output(l, n)
        s = np.zeros(6)
        for i in range(0, n, step):
            a64, b64 = a[i:i + step].astype(np.float64), b[i:i + step].astype(np.float64)
            ok = np.isfinite(a64) & np.isfinite(b64)
            d = np.where(ok, a64 - b64, 0.0)
            r = np.where(ok, b64, 0.0)
            s[0] += ok.sum(); s[1] += ok.size - ok.sum(); s[2] += d.sum(); s[3] += (d * d).sum(); s[4] += (r * r).sum()
            s[5] = max(s[5], np.abs(d).max())
        out[l] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--calib", type=int, default=256)
    ap.add_argument("--sweeps", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    topo, synth, engine, quantize, capi = pkg("topology"), pkg("synth"), pkg("engine"), pkg("quantize"), pkg("capi")
    in_chw, layers = topo.MODELS["AlexNet"][:2]
    dense = synth.make_dense_params(in_chw, layers, seed=a.seed)
    ids = sorted(dense)
    n = a.batch
    imgs = synth.make_images(n, in_chw, seed=a.seed + 1)
    cal = synth.make_images(a.calib, in_chw, seed=a.seed + 2)

    ref = engine.QcnnEngine(0)
    ref.set_option(capi.OPT_KEEP_ALL, 1)
    ref.load_dense_model(in_chw, layers, dense, n)
    eng = engine.QcnnEngine(0)
    t0 = time.perf_counter()
    calib = quantize.calibrate(eng, in_chw, layers, dense, cal, chunk=32, resident=True)
    p_km, st_km = quantize.quantize_model(eng, in_chw, layers, dense)
    p_ec, st_ec = quantize.quantize_model(eng, in_chw, layers, dense, calib=calib, sweeps=a.sweeps)
    print("# calibrated on %d images and quantised twice in %.1f s" % (a.calib, time.perf_counter() - t0), file=sys.stderr, flush=True)

    eng.set_option(capi.OPT_KEEP_ALL, 1)
    reports, agrees = {}, {}
    for name, p in (("kmeans", p_km), ("ec", p_ec)):                 # the error-corrected model last: the timings below run on it
        eng.load_model(in_chw, layers, p, n)
        reports[name], agrees[name] = quantize.response_report(eng, ref, [imgs])
    maps = quantize.default_report_maps(layers)

    print("layer  map  weight rel_err (k-means / EC)   EC obj before -> after     propagated rel_err (k-means / EC)")
    rows = []
    for i in ids:
        km, ec = reports["kmeans"][i + 1], reports["ec"][i + 1]
        rows.append(dict(layer=i, map=i + 1, weight_rel_err_kmeans=st_km[i]["rel_err"], weight_rel_err_ec=st_ec[i]["rel_err"],
                         ec_obj_init=st_ec[i]["obj_init"], ec_obj=st_ec[i]["obj"], rel_err_kmeans=km["rel_err"], rel_err_ec=ec["rel_err"],
                         mean_d_ec=ec["mean_d"], max_abs_d_ec=ec["max_abs_d"], nonfinite=km["nonfinite"] + ec["nonfinite"]))
        print("%5d %4d  %.4f / %.4f                 %.4g -> %.4g        %.4f / %.4f"
              % (i, i + 1, st_km[i]["rel_err"], st_ec[i]["rel_err"], st_ec[i]["obj_init"], st_ec[i]["obj"], km["rel_err"], ec["rel_err"]))
    L = len(layers)
    print("last map %d (probabilities): rel_err %.4f / %.4f" % (L, reports["kmeans"][L]["rel_err"], reports["ec"][L]["rel_err"]))
    print("agree k-means: %s" % agrees["kmeans"])
    print("agree EC:      %s" % agrees["ec"])

    # the two routes on the maps both engines hold now (the error-corrected model's last forward)
    floats = sum(int(np.prod(eng.fm_dims(l))) for l in maps) * n
    dev = lambda: {l: eng.map_diff(ref, l, n) for l in maps}
    dev()                                                            # warm-up: the scratch is allocated
    ms = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        got = dev()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    t0 = time.perf_counter()
    host = host_route(np, eng, ref, maps, n)
    host_s = time.perf_counter() - t0
    worst = max(abs(got[l]["sum_d2"] - host[l][3]) / host[l][3] for l in maps)
    same = all(got[l]["count"] == host[l][0] and got[l]["max_abs_d"] == host[l][5] for l in maps)
    print("one batch of %d images, %d maps, 2 x %.2f GB of maps: device report %.2f ms (min %.2f, max %.2f of %d), host route %.2f s; "
          "sum_d2 agrees to %.1e relative, count and max_abs_d %s"
          % (n, len(maps), floats * 4 / 1e9, ms[len(ms) // 2], ms[0], ms[-1], len(ms), host_s, worst, "equal" if same else "DIFFER"))
    print(json.dumps(dict(model="AlexNet", batch=n, calib=a.calib, sweeps=a.sweeps, layers=rows,
                          last_map=dict(rel_err_kmeans=reports["kmeans"][L]["rel_err"], rel_err_ec=reports["ec"][L]["rel_err"]),
                          agree_kmeans=agrees["kmeans"], agree_ec=agrees["ec"], maps=maps, map_bytes_each=floats * 4,
                          device_ms_median=round(ms[len(ms) // 2], 3), device_ms_min_max=[round(ms[0], 3), round(ms[-1], 3)],
                          host_route_s=round(host_s, 3), sum_d2_rel_diff=worst, count_and_max_equal=bool(same))), flush=True)
    eng.close()
    ref.close()


if __name__ == "__main__":
    main()
