"""Dense weights -> Q-CNN parameters: the quantisation step whose results the reference ships (its parameters came from
MATLAB code that was not released), run on the GPU through ``QcnnEngine.quantize_layer`` (qcnn_quantize_layer).

``decode_layer``        the inverse map: sub-codebooks + assignments -> dense weights in the convKnl / fcntWei file layout
``quantize_model``      every conv / FC layer of a dense parameter set (synth.make_dense_params form) at the shipped layout
                        rule (synth.quant_spec); returns the params dict engine.load_model, synth.write_param_dir and
                        pyoracle.COracle.set_params take, plus per-layer statistics
``calibrate``           second moments of every conv / FC layer's input on calibration images (the dense network's own
                        feature maps), for the error-corrected refinement ``quantize_model(..., calib=...)`` runs after k-means
``calibrate_u8``        the same on 8-bit source images streamed from host memory, accumulated on the device
``quantize_param_dir``  reads ``<pfx>.biasVec`` + ``convKnl`` / ``fcntWei`` files, writes ``biasVec`` + ``ctrdLst`` +
                        ``asmtLst.cbn`` (minimum bits, CaffePara::CalcBitCntPerEle) for the reference's LoadLayerPara

An FC layer is a conv layer with kh = kw = 1 and Cin = D: its weights [Ct][D] are the bytes of [Ct][D][1][1], its
assignments [Ct][M] those of [Ct][1][1][M].  There is no CPU path: without a GPU the engine cannot be created.
"""
from __future__ import annotations

import os
import time

import numpy as np

from . import capi, fileio, synth, topology
from .engine import DEFAULT_EC_RIDGE, DEFAULT_EC_SWEEPS, DEFAULT_MAX_ITER, QcnnEngine
from .topology import CONV, FCNT


def decode_layer(ctrd, asmt, wshape):
    """Dense weights [Ct][Cin][kh][kw] (len(wshape) == 4) or [Ct][D] (len 2) from ctrd [M][K][Cs] and 0-based assignments in
    file order ([Ct][kh][kw][M] / [Ct][M]): W[ct, m*Cs + j, y, x] = ctrd[m, asmt[ct, y, x, m], j] for m*Cs + j < Cin."""
    ctrd = np.asarray(ctrd, np.float32)
    m, _, cs = ctrd.shape
    wshape = tuple(int(x) for x in wshape)
    if len(wshape) == 4:
        ct, cin, kh, kw = wshape
    elif len(wshape) == 2:
        (ct, cin), kh, kw = wshape, 1, 1
    else:
        raise ValueError("wshape must have 2 or 4 dims, got %r" % (wshape,))
    a = np.asarray(asmt).astype(np.intp).reshape(ct, kh, kw, m)
    sub = ctrd[np.arange(m)[None, None, None, :], a]                  # [Ct][kh][kw][M][Cs]
    dense = sub.reshape(ct, kh, kw, m * cs)[..., :cin]                 # [Ct][kh][kw][Cin]
    return np.ascontiguousarray(dense.transpose(0, 3, 1, 2)).reshape(wshape)


def _layer_stats(w, ctrd, asmt, st, seconds):
    wd = decode_layer(ctrd, asmt, w.shape).astype(np.float64)
    w64 = np.asarray(w, np.float64)
    den = np.sqrt((w64 * w64).sum())
    rel = float(np.sqrt(((w64 - wd) ** 2).sum()) / den) if den > 0 else 0.0
    return dict(st, rel_err=rel, seconds=seconds)


def layer_geom(layers, i):
    """dict(grp, kh, kw, stride, pad) of conv / FC layer i as QcnnEngine.calib_gram takes it (FC: a 1x1 window on a 1x1 map)."""
    ly = layers[i]
    if ly["type"] == CONV:
        return dict(grp=ly["grp"], kh=ly["knl"], kw=ly["knl"], stride=ly["stride"], pad=ly["pad"])
    if ly["type"] == FCNT:
        return dict(grp=1, kh=1, kw=1, stride=1, pad=0)
    raise ValueError("layer %d is neither conv nor FC" % i)


def layer_input(layers, i, fm_nhwc):
    """Feature map i ([n][H][W][C], QcnnEngine.layer_output) as layer i consumes it — what run_layer and calib_gram take: a conv
    layer reads it as it is, an FC layer the flat vector in the reference's order (channel-major: [n][C][H][W] flattened)."""
    x = np.asarray(fm_nhwc, np.float32)
    if layers[i]["type"] == FCNT:
        x = x.transpose(0, 3, 1, 2).reshape(x.shape[0], 1, 1, -1)
    return np.ascontiguousarray(x)


def _read_resident(eng, dense):
    try:
        return {i: eng.calib_read(i)[0] for i in sorted(dense)}
    finally:
        eng.calib_end()


def calibrate(eng, in_chw, layers, dense, imgs, chunk=32, resident=False):
    """{layer: gram [grp][P][P] float64} for every layer of ``dense``: the dense model (load_dense_model, every feature map kept)
    forwards ``imgs`` [n][C][H][W] in chunks, and each conv / FC layer's INPUT map goes to ``eng.calib_gram``, accumulating.
    Every layer sees the dense network's activations, so layers are corrected independently of each other.  Loads a model
    into ``eng``: whatever it held before is replaced, and QCNN_OPT_KEEP_ALL is left at 1 (the library's default).
    ``resident=True``: the sums are accumulated on the device behind every chunk's forward (eng.calib_begin on every layer of
    ``dense``) and read once at the end — no map travels to the host and back; same dict, equal within the kernels' bound."""
    imgs = np.ascontiguousarray(imgs, np.float32)
    chunk = max(1, min(int(chunk), len(imgs)))
    eng.set_option(capi.OPT_KEEP_ALL, 1)
    eng.load_dense_model(in_chw, layers, dense, chunk)
    if resident:
        eng.calib_begin(sorted(dense))
        try:
            for n0 in range(0, len(imgs), chunk):
                eng.forward_host(imgs[n0:n0 + chunk], want_prob=False, want_top5=False)
        except BaseException:
            eng.calib_end()
            raise
        return _read_resident(eng, dense)
    grams = {}
    for n0 in range(0, len(imgs), chunk):
        part = imgs[n0:n0 + chunk]
        eng.forward_host(part, want_prob=False, want_top5=False)
        for i in sorted(dense):
            x = layer_input(layers, i, eng.layer_output(i, len(part)))
            grams[i] = eng.calib_gram(x, layer_geom(layers, i), grams.get(i))
    return grams


def calibrate_u8(eng, in_chw, layers, dense, batches, full_hw, mean=None, views=None, mode="strict", max_batch=None):
    """``calibrate(resident=True)`` on 8-bit source images streamed from host memory (eng.forward_u8_host_batches): ``batches``
    is what engine.split_batches returns ([(flat, descs, labels)], B, G, R or YCbCr descriptors; the labels are not used),
    ``full_hw`` / ``mean`` / ``views`` / ``mode`` as forward_u8_host_batches takes them.  Every view of every image is one
    calibration input.  ``max_batch``: batch slots the model is committed for (default: the largest batch x views)."""
    V = 1 if views is None else len(views)
    if max_batch is None:
        max_batch = max(len(b[1]) for b in batches) * V
    eng.set_option(capi.OPT_KEEP_ALL, 1)
    eng.load_dense_model(in_chw, layers, dense, int(max_batch))
    eng.calib_begin(sorted(dense))
    try:
        eng.forward_u8_host_batches([(b[0], b[1]) for b in batches], full_hw, mean, views, mode, want=(False, False, False))
    except BaseException:
        eng.calib_end()
        raise
    return _read_resident(eng, dense)


def quantize_model(eng, in_chw, layers, dense, spec=None, max_iter=DEFAULT_MAX_ITER, calib=None, sweeps=DEFAULT_EC_SWEEPS,
                   ridge=DEFAULT_EC_RIDGE):
    """Quantise every layer of ``dense`` ({layer: dict(bias, weights)}, synth.make_dense_params / the convKnl, fcntWei files)
    with ``eng.quantize_layer`` at ``spec`` (default synth.quant_spec: conv Cs = 8, K = 128; hidden FC Cs = 4, K = 32;
    classifier Cs = 1, K = 16).  Returns (params {layer: dict(bias, ctrd, asmt, bits)}, stats {layer: dict(sse_init, sse,
    iters, unconverged, rel_err = |W - W_hat| / |W|, seconds = wall time of the call incl. copies)}).  With ``calib``
    ({layer: gram}, the result of ``calibrate``) every layer in it is then refined by ``eng.quantize_layer_ec`` (``sweeps``,
    ``ridge``) from the k-means result, and its stats gain obj_init, obj (response error e^T G e before / after), sweeps and
    changed; without it the k-means result is returned as it always was."""
    spec = spec or synth.quant_spec(in_chw, layers)
    params, stats = {}, {}
    for i in sorted(dense):
        if i not in spec:
            raise ValueError("layer %d has dense weights but no quantisation shape in spec" % i)
        s = spec[i]
        w = np.ascontiguousarray(dense[i]["weights"], np.float32)
        t0 = time.perf_counter()
        ctrd, asmt, st = eng.quantize_layer(w, s["M"], s["K"], s["Cs"], max_iter=max_iter)
        if calib is not None and i in calib:
            grp = layers[i]["grp"] if layers[i]["type"] == CONV else 1
            ctrd, asmt, ec = eng.quantize_layer_ec(w, s["M"], s["K"], s["Cs"], calib[i], ctrd, asmt, grp=grp, sweeps=sweeps, ridge=ridge)
            st = dict(st, obj_init=ec["obj_init"], obj=ec["obj"], sweeps=ec["sweeps"], changed=[int(x) for x in ec["changed"]])
        dt = time.perf_counter() - t0
        params[i] = dict(bias=np.ascontiguousarray(dense[i]["bias"], np.float32), ctrd=ctrd, asmt=asmt,
                         bits=fileio.min_bits(asmt))
        stats[i] = _layer_stats(w, ctrd, asmt, st, dt)
    return params, stats


def _forward_float(eng, batch):
    x = np.ascontiguousarray(batch, np.float32)
    return len(x), eng.forward_host(x, want_prob=False)[1]


def default_report_maps(layers):
    """The maps response_report compares unless told otherwise: the output map i + 1 of every conv / FC layer i, and the last."""
    maps = [i + 1 for i, ly in enumerate(layers) if ly["type"] in (CONV, FCNT)]
    return maps if len(layers) in maps else maps + [len(layers)]


def response_report(eng, ref, batches, maps=None, forward=None, per_channel=False):
    """How far every feature map of the model in ``eng`` (the subject, e.g. a quantised network) is from the same map of the
    model in ``ref`` (e.g. the dense network) on the same inputs, the error of the layers in front carried along, and how often
    the two agree on the answer — compared on the device where the forwards left the maps (QcnnEngine.map_diff).  For every
    batch: ``forward(ref, batch)`` then ``forward(eng, batch)``, each returning (n, top5 [n][5]) — default: forward_host on a
    float [n][C][H][W] array; pass a callable for 8-bit or YCbCr sources, one batch per call (only the last batch's maps
    survive a *_host_batches call) — then ``eng.map_diff(ref, l, n)`` for every l of ``maps`` (default_report_maps), added
    over the batches on the host in fp64 (sums add, max_abs_d takes the maximum).  Returns (report {l: dict with map_diff's
    keys, derived from the accumulated sums; with per_channel=True also ``channels`` [C][6], accumulated the same way, and the
    totals are then the fold of those rows in ascending channel order, to the bit}, agree dict(n, top1_equal = images whose
    first predictions are equal, ref_top1_in_top5 = images whose reference first prediction is among the subject's five)).
    Both engines need OPT_KEEP_ALL = 1 for maps the fast path fuses away: such a map raises QcnnError, it is never skipped."""
    from .engine import map_diff_summary
    forward = forward or _forward_float
    maps = [int(l) for l in (default_report_maps(eng.layers) if maps is None else maps)]
    fields = capi.MAP_DIFF_FIELDS
    imax = fields.index("max_abs_d")
    sums = {l: dict.fromkeys(fields, 0.0) for l in maps}
    chans = {}
    agree = dict(n=0, top1_equal=0, ref_top1_in_top5=0)
    for batch in batches:
        n_ref, t_ref = forward(ref, batch)
        n, t_eng = forward(eng, batch)
        if n != n_ref:
            raise ValueError("response_report: the two forwards ran %d and %d images" % (n_ref, n))
        t_ref, t_eng = np.asarray(t_ref).reshape(n, -1), np.asarray(t_eng).reshape(n, -1)
        agree["n"] += int(n)
        agree["top1_equal"] += int(np.count_nonzero(t_eng[:, 0] == t_ref[:, 0]))
        agree["ref_top1_in_top5"] += int(np.count_nonzero((t_eng == t_ref[:, :1]).any(axis=1)))
        for l in maps:
            r = eng.map_diff(ref, l, n, per_channel=per_channel)
            s = sums[l]
            for f in fields:
                s[f] = max(s[f], float(r[f])) if f == "max_abs_d" else s[f] + float(r[f])
            if per_channel:
                ch = np.asarray(r["channels"], np.float64)
                if l not in chans:
                    chans[l] = ch.copy()
                else:
                    mx = np.maximum(chans[l][:, imax], ch[:, imax])
                    chans[l] += ch
                    chans[l][:, imax] = mx
    for l, ch in chans.items():                        # per_channel: the totals are the fold of the rows handed back, to the bit
        for j, f in enumerate(fields):
            sums[l][f] = float(ch[:, j].max()) if j == imax else float(np.add.accumulate(ch[:, j])[-1])
    report = {l: map_diff_summary(sums[l]) for l in maps}
    for l, ch in chans.items():
        report[l]["channels"] = ch
    return report, agree


def _model_tables(model):
    if isinstance(model, str):
        in_chw, layers, _, _ = topology.MODELS[model]
        return in_chw, layers
    return model


def read_dense_param_dir(dir_path, prefix, layers):
    """{layer: dict(bias, weights)} from ``<pfx>.biasVec.NN.bin`` + ``convKnl.NN.bin`` / ``fcntWei.NN.bin``
    (the files CaffePara::LoadLayerPara(false, ..) reads, src/CaffePara.cc:290-302)."""
    out = {}
    for i, ly in enumerate(layers):
        if ly["type"] not in (CONV, FCNT):
            continue
        bias = fileio.read_bin(fileio.param_path(dir_path, prefix, "biasVec", i + 1, "bin"), np.float32)
        kind = "convKnl" if ly["type"] == CONV else "fcntWei"
        w = fileio.read_bin(fileio.param_path(dir_path, prefix, kind, i + 1, "bin"), np.float32)
        out[i] = dict(bias=bias.reshape(-1), weights=w)
    return out


def quantize_param_dir(src_dir, src_pfx, dst_dir, dst_pfx, model, eng=None, spec=None, max_iter=DEFAULT_MAX_ITER, calib_images=None,
                       sweeps=DEFAULT_EC_SWEEPS, ridge=DEFAULT_EC_RIDGE, calib_sources=None):
    """Quantise a dense parameter directory into a Q-CNN one.  ``model``: a name of topology.MODELS or (in_chw, layers).
    ``eng``: anything with QcnnEngine.quantize_layer's signature (default: a QcnnEngine on device 0).  ``calib_images``
    ([n][C][H][W]): error-corrected on them (calibrate + quantize_model(calib=...)); ``eng`` then loses the model it held.
    ``calib_sources`` = (batches, full_hw, mean, views, mode) instead: error-corrected on 8-bit sources (calibrate_u8).
    Returns the stats of quantize_model."""
    in_chw, layers = _model_tables(model)
    dense = read_dense_param_dir(src_dir, src_pfx, layers)
    own = eng is None
    if own:
        eng = QcnnEngine(0)
    try:
        if calib_images is not None and calib_sources is not None:
            raise ValueError("quantize_param_dir: calib_images or calib_sources, not both")
        calib = calibrate(eng, in_chw, layers, dense, calib_images) if calib_images is not None else None
        if calib_sources is not None:
            batches, full_hw, mean, views, mode = calib_sources
            calib = calibrate_u8(eng, in_chw, layers, dense, batches, full_hw, mean, views, mode)
        params, stats = quantize_model(eng, in_chw, layers, dense, spec=spec, max_iter=max_iter, calib=calib, sweeps=sweeps, ridge=ridge)
    finally:
        if own:
            eng.close()
    os.makedirs(dst_dir, exist_ok=True)
    synth.write_param_dir(dst_dir, dst_pfx, params)
    return stats
