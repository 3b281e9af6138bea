"""The two-piece fp16 split behind QCNN_OPT_DEC_BF16SPLIT = 2, modelled in numpy (f16split_model.py): the remainder
subtraction is exact, x1 + x2 carries Sx x to 2^-22 (or to the subnormal quantum), the three cross terms kept by
k_conv_dec_nchw_f16 reproduce a product within 3 x 2^-22 of its magnitude plus the subnormal term, the range predicate
catches NaN / Inf / anything beyond X_MAX and nothing at or below it, and the decoder's scale rule."""
import numpy as np

import f16split_model as fm

SX, XMAX = fm.SX, fm.XMAX
U2 = 2.0 ** -22                                         # u^2, u = 2^-11


def values():
    """test_bf16split_cpu.py's families restricted to the scaled range |x| <= X_MAX, plus the edges of the range, both zeros and
    values whose second (or first) piece is subnormal in fp16."""
    rng = np.random.default_rng(5)
    x_above = np.nextafter(np.float32(XMAX), np.float32(np.inf))
    v = [rng.standard_normal(20000).astype(np.float32),
         (rng.standard_normal(5000) * 1e-30).astype(np.float32),
         rng.integers(-255, 256, 5000).astype(np.float32) - 0.5,
         np.array([0.0, -0.0, 1.0, -1.0, XMAX, -XMAX, 1.17549435e-38, np.float32(1) + np.float32(2 ** -23)], np.float32),
         rng.uniform(-1, 1, 5000).astype(np.float32).view(np.uint32).__or__(np.uint32(0x00FFFF)).view(np.float32),
         rng.uniform(-XMAX, XMAX, 5000).astype(np.float32),
         # second piece subnormal: Sx x just above a small fp16 number (remainder below 2^-14); first piece subnormal: |Sx x| < 2^-14
         ((2.0 ** rng.integers(-13, -3, 2000)) * (1 + 2.0 ** -12 * rng.uniform(0.1, 1, 2000)) / SX).astype(np.float32),
         (rng.uniform(-1, 1, 2000) * 2.0 ** -15 / SX).astype(np.float32),
         (10.0 ** rng.uniform(-6, -3, 2000) * rng.choice([-1, 1], 2000)).astype(np.float32)]
    v = np.concatenate(v)
    return v[~fm.out_of_range(v)], x_above


def test_two_piece_split():
    x, _ = values()
    x1, x2, r = fm.split2(x, SX)
    s64 = x.astype(np.float64) * SX
    assert np.isfinite(x1).all() and np.isfinite(x2).all()
    assert np.array_equal(r.astype(np.float64), s64 - x1)                 # the remainder subtraction is exact in fp32
    for p in (x1, x2):                                                    # every piece is an fp16 value
        assert np.array_equal(p.astype(np.float16).astype(np.float32), p)
    err = np.abs(s64 - (x1.astype(np.float64) + x2)) / SX                 # |x - (x1 + x2) / Sx|
    assert (err <= np.maximum(U2 * np.abs(x.astype(np.float64)), fm.ETA / SX)).all(), float(err.max())
    assert np.array_equal(np.signbit(x1), np.signbit(x))                  # +-0 keep their sign in the first piece
    sub2 = (np.abs(x2) < 2.0 ** -14) & (x2 != 0)
    assert sub2.any() and ((np.abs(x1) < 2.0 ** -14) & (x1 != 0)).any()   # the subnormal families are there


def test_three_terms_bound_the_product_error():
    rng = np.random.default_rng(6)
    x, _ = values()
    for sw, wscale in ((2.0 ** 17, 0.05), (2.0 ** 13, 1.0), (2.0 ** 30, 1e-5)):
        w = (rng.standard_normal(x.size) * wscale).astype(np.float32)
        w = np.clip(w, -2.0 ** 14 / sw * 0.999, 2.0 ** 14 / sw * 0.999).astype(np.float32)   # the decoder's scale keeps |Sw w| < 2^14
        w[::7] = (w[::7] * 2.0 ** -rng.integers(8, 24, w[::7].size)).astype(np.float32)      # small code words: subnormal pieces
        x1, x2, _ = (p.astype(np.float64) for p in fm.split2(x, SX))
        w1, w2, _ = (p.astype(np.float64) for p in fm.split2(w, sw))
        three = (x2 * w1 + x1 * w2 + x1 * w1) / (SX * sw)
        exact = x.astype(np.float64) * w
        bound = 3 * U2 * np.abs(exact) + fm.ETA * (np.abs(w) / SX + np.abs(x) / sw) * (1 + 2 * U2)
        err = np.abs(three - exact)
        assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())


def test_range_predicate():
    _, x_above = values()
    inside = np.array([0.0, -0.0, 1.0, XMAX, -XMAX, 1e-45], np.float32)
    outside = np.array([x_above, -x_above, 2 * XMAX, 1e30, -1e30, np.inf, -np.inf, np.nan, -np.nan], np.float32)
    assert not fm.out_of_range(inside).any()
    assert fm.out_of_range(outside).all()
    x1, x2, _ = fm.split2(inside, SX)                                     # everything inside splits into finite pieces
    assert np.isfinite(x1).all() and np.isfinite(x2).all() and np.abs(x1).max() <= 65504.0
    assert SX * XMAX <= 65504.0 and XMAX >= 512.0


def test_weight_scale_rule():
    assert fm.weight_scale(0.0) == 0.0                                    # all code words zero: the bf16 form
    assert fm.weight_scale(1e-45) == 0.0 and fm.weight_scale(1.1e-38) == 0.0   # denormal
    assert fm.weight_scale(np.inf) == 0.0 and fm.weight_scale(np.nan) == 0.0
    assert fm.weight_scale(1e30) == 0.0                                   # Sx Sw < 1: bias Sx Sw would not be exact
    assert fm.weight_scale(1.0) == 2.0 ** 13
    assert fm.weight_scale(1.9999) == 2.0 ** 13 and fm.weight_scale(2.0) == 2.0 ** 12
    assert fm.weight_scale(1e-30) == 2.0 ** 113                            # floor(log2 1e-30) = -100
    assert fm.weight_scale(2.0 ** -107) == 2.0 ** 120 and fm.weight_scale(2.0 ** -108) == 0.0
    assert fm.weight_scale(2.0 ** 19) == 2.0 ** -6 and fm.weight_scale(2.0 ** 20) == 0.0
    rng = np.random.default_rng(7)
    for m in 10.0 ** rng.uniform(-30, 5.5, 200):                          # the largest first piece lands in [2^13, 2^14]
        sw = fm.weight_scale(m)
        w1 = float(np.float32(np.float32(m) * np.float32(sw)).astype(np.float16))
        assert sw > 0 and 2.0 ** 13 <= w1 <= 2.0 ** 14, (m, sw, w1)
        assert np.log2(sw) == np.round(np.log2(sw)) and 1.0 <= SX * sw <= 2.0 ** 126
    assert fm.weight_scale(1.0, np.inf) == 0.0 and fm.weight_scale(1.0, np.nan) == 0.0
    assert fm.weight_scale(1.0, 2.0 ** 81) == 2.0 ** 13 and fm.weight_scale(1.0, 2.0 ** 82) == 0.0   # |bias| Sx Sw <= 2^100
