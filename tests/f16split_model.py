"""The two-piece fp16 form of the decoded first layer (QCNN_OPT_DEC_BF16SPLIT = 2, k_conv_dec_nchw_f16) modelled in numpy: the
split, the scale rule of the decoder, the range predicate of the guard and the per-output error bound.  Shared by
test_f16split_cpu.py and test_gpu_dec_f16split.py; the constants are read from the kernel header, the formulas are the
kernels' (csrc/qcnn_kernels.h qk_f16_weight_scale, csrc/qcnn_decoded.hip split_f16x8 / k_decode_weights_f16).

Error of one output.  With u = 2^-11 and pieces that are normal fp16 numbers, Sx x = (x1 + x2)(1 + d), |d| <= u^2, likewise
Sw w, and the three kept terms x2 w1 + x1 w2 + x1 w1 miss (x1 + x2)(w1 + w2) by x2 w2 <= u^2 |x1 w1|: one product is within
3 u^2 |x w| of exact.  A piece in fp16's subnormal range is rounded to a multiple of 2^-24 instead: an absolute ETA per piece in
scaled units, i.e. ETA (|w| / Sx + |x| / Sw) per product after the scales are taken out.  The 3 n products and the bias are
added in fp32, each addition rounding a partial sum that |bias| + sum |x w| bounds: gamma(3 n + 1) of that (n = the padded k;
table_probe.dec_dense_rel has the same shape for the bf16 form, 2^-22 + gamma(6 n + 1), with the bias inside its magnitude too).
Both scalings are by powers of two and exact."""
import os
import re

import numpy as np

from conftest import ROOT

U32 = 2.0 ** -24


def _define(name):
    text = open(os.path.join(ROOT, "quantized-cnn_amd", "csrc", "qcnn_kernels.h")).read()
    return float(re.search(r"#define\s+%s\s+([0-9.]+)f?" % name, text).group(1))


SX = _define("QK_F16_SX")
XMAX = _define("QK_F16_XMAX")
# v_mfma_f32_16x16x32_f16 takes subnormal fp16 inputs as they are (the matrix instructions do not flush their 16-bit inputs;
# test_gpu_dec_f16split.py::test_tiny_inputs holds the kernel to this value): a subnormal piece costs its rounding to 2^-24,
# at most half of that
ETA = 2.0 ** -25


def gamma(m):
    return m * U32 / (1.0 - m * U32)


def split2(x, scale):
    """x (fp32) -> x1, x2, r as fp32 arrays: x1 = f16(scale x), r = scale x - x1 in fp32, x2 = f16(r); round to nearest even."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float32)
        x1 = s.astype(np.float16).astype(np.float32)
        r = (s - x1).astype(np.float32)
        x2 = r.astype(np.float16).astype(np.float32)
    return x1, x2, r


def out_of_range(x):
    """The guard's predicate, the kernel's negated compare: true for NaN too."""
    with np.errstate(invalid="ignore"):
        return ~(np.abs(np.asarray(x, np.float32)) <= np.float32(XMAX))


def weight_scale(max_w, max_bias=0.0):
    """qk_f16_weight_scale on the largest |code word| and |bias|: Sw, or 0.0 when the layer keeps the bf16 form."""
    mw = int(np.abs(np.float32(max_w)).view(np.uint32))
    mb = int(np.abs(np.float32(max_bias)).view(np.uint32))
    e = (mw >> 23) - 127
    if mw >= 0x7F800000 or mw < 0x00800000 or e < -107 or e > 19 or mb >= 0x7F800000:
        return 0.0
    sw = np.float32(2.0) ** np.float32(13 - e)
    with np.errstate(over="ignore"):
        ok = np.float32(np.abs(np.float32(max_bias))) * (np.float32(SX) * sw) <= np.float32(2.0) ** np.float32(100)
    return float(sw) if ok else 0.0


def layer_scale(params, cin):
    """Sw of a one-sub-space conv layer's parameters (synth.make_params entry): the largest |code word| any assignment names."""
    ctrd = np.asarray(params["ctrd"], np.float32)[0]                 # [K, Cs]
    used = ctrd[np.unique(np.asarray(params["asmt"]))][:, :cin]
    return weight_scale(np.abs(used).max() if used.size else 0.0, np.abs(params["bias"]).max())


def output_bound(mag_xw, sum_abs_w, sum_abs_x, abs_bias, n_pad, sw, eta=ETA):
    """Per-output bound: sum_k [3 2^-22 |x_k w_k| + eta (|w_k| / Sx + |x_k| / Sw)] + gamma(3 n + 1) (|bias| + sum_k |x_k w_k|)."""
    return 3.0 * 2.0 ** -22 * mag_xw + eta * (sum_abs_w / SX + sum_abs_x / sw) + gamma(3 * n_pad + 1) * (abs_bias + mag_xw)


def padded_k(cin, knl, ct):
    """The k slots one output sums (qk_conv_dec_nchw_split_shape's Kb): run order — ceil(knl / 4) runs of 4 columns per kernel row,
    pairs of runs padded to steps of 32 — where knl >= 4 and the planes fit LDS, else the window padded to a multiple of 32."""
    nr = (knl + 3) // 4 if knl >= 4 else 0
    if nr:
        kb = (cin * knl * nr + 7) // 8 * 32
        if kb * ct * 4 + (kb // 4 + 8) * 4 <= 160 * 1024:
            return kb
    return (cin * knl * knl + 31) // 32 * 32


def abs_sums(x_nhwc, params, knl, stride, cin):
    """(sum_k |w_k| per channel [Ct], sum_k |x_k| per output [n, Ho, Wo]) of an unpadded one-sub-space conv layer."""
    x = np.abs(np.asarray(x_nhwc, np.float32).astype(np.float64))
    n, H, W, _ = x.shape
    Ho, Wo = (H - knl) // stride + 1, (W - knl) // stride + 1
    ct = params["asmt"].shape[0]
    a = np.asarray(params["asmt"]).reshape(ct, knl, knl).astype(np.int64)
    w = np.abs(np.asarray(params["ctrd"], np.float32)[0][a][..., :cin].astype(np.float64))
    sx = np.zeros((n, Ho, Wo))
    xs = x.sum(-1)
    for kh in range(knl):
        for kw in range(knl):
            sx += xs[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride]
    return w.sum(axis=(1, 2, 3)), sx
