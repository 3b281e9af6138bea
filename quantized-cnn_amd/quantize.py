"""Dense weights -> Q-CNN parameters: the quantisation step whose results the reference ships (its parameters came from
MATLAB code that was not released), run on the GPU through ``QcnnEngine.quantize_layer`` (qcnn_quantize_layer).

``decode_layer``        the inverse map: sub-codebooks + assignments -> dense weights in the convKnl / fcntWei file layout
``quantize_model``      every conv / FC layer of a dense parameter set (synth.make_dense_params form) at the shipped layout
                        rule (synth.quant_spec); returns the params dict engine.load_model, synth.write_param_dir and
                        pyoracle.COracle.set_params take, plus per-layer statistics
``quantize_param_dir``  reads ``<pfx>.biasVec`` + ``convKnl`` / ``fcntWei`` files, writes ``biasVec`` + ``ctrdLst`` +
                        ``asmtLst.cbn`` (minimum bits, CaffePara::CalcBitCntPerEle) for the reference's LoadLayerPara

An FC layer is a conv layer with kh = kw = 1 and Cin = D: its weights [Ct][D] are the bytes of [Ct][D][1][1], its
assignments [Ct][M] those of [Ct][1][1][M].  There is no CPU path: without a GPU the engine cannot be created.
"""
from __future__ import annotations

import os
import time

import numpy as np

from . import fileio, synth, topology
from .engine import DEFAULT_MAX_ITER, QcnnEngine
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


def quantize_model(eng, in_chw, layers, dense, spec=None, max_iter=DEFAULT_MAX_ITER):
    """Quantise every layer of ``dense`` ({layer: dict(bias, weights)}, synth.make_dense_params / the convKnl, fcntWei files)
    with ``eng.quantize_layer`` at ``spec`` (default synth.quant_spec: conv Cs = 8, K = 128; hidden FC Cs = 4, K = 32;
    classifier Cs = 1, K = 16).  Returns (params {layer: dict(bias, ctrd, asmt, bits)}, stats {layer: dict(sse_init, sse,
    iters, unconverged, rel_err = |W - W_hat| / |W|, seconds = wall time of the call incl. copies)})."""
    spec = spec or synth.quant_spec(in_chw, layers)
    params, stats = {}, {}
    for i in sorted(dense):
        if i not in spec:
            raise ValueError("layer %d has dense weights but no quantisation shape in spec" % i)
        s = spec[i]
        w = np.ascontiguousarray(dense[i]["weights"], np.float32)
        t0 = time.perf_counter()
        ctrd, asmt, st = eng.quantize_layer(w, s["M"], s["K"], s["Cs"], max_iter=max_iter)
        dt = time.perf_counter() - t0
        params[i] = dict(bias=np.ascontiguousarray(dense[i]["bias"], np.float32), ctrd=ctrd, asmt=asmt,
                         bits=fileio.min_bits(asmt))
        stats[i] = _layer_stats(w, ctrd, asmt, st, dt)
    return params, stats


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


def quantize_param_dir(src_dir, src_pfx, dst_dir, dst_pfx, model, eng=None, spec=None, max_iter=DEFAULT_MAX_ITER):
    """Quantise a dense parameter directory into a Q-CNN one.  ``model``: a name of topology.MODELS or (in_chw, layers).
    ``eng``: anything with QcnnEngine.quantize_layer's signature (default: a QcnnEngine on device 0).  Returns the stats of
    quantize_model."""
    in_chw, layers = _model_tables(model)
    dense = read_dense_param_dir(src_dir, src_pfx, layers)
    own = eng is None
    if own:
        eng = QcnnEngine(0)
    try:
        params, stats = quantize_model(eng, in_chw, layers, dense, spec=spec, max_iter=max_iter)
    finally:
        if own:
            eng.close()
    os.makedirs(dst_dir, exist_ok=True)
    synth.write_param_dir(dst_dir, dst_pfx, params)
    return stats
