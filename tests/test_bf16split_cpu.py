"""The exact three-piece bf16 split behind QCNN_OPT_DEC_BF16SPLIT, modelled in numpy: x = x1 + x2 + x3 exactly, and the
six cross terms kept by k_conv_dec_nchw_split reproduce a product within 2^-22 of its magnitude."""
import numpy as np


def bf16_rn(x):
    """fp32 -> nearest-even bf16, returned as fp32 (finite inputs)."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, np.float32)
    x1 = bf16_rn(x)
    r = (x - x1).astype(np.float32)
    x2 = bf16_rn(r)
    x3 = bf16_rn((r - x2).astype(np.float32))
    return x1, x2, x3


def values():
    rng = np.random.default_rng(5)
    v = [rng.standard_normal(20000).astype(np.float32),
         (rng.standard_normal(5000) * 1e30).astype(np.float32),
         (rng.standard_normal(5000) * 1e-30).astype(np.float32),
         rng.integers(-255, 256, 5000).astype(np.float32) - 0.5,
         np.array([0.0, -0.0, 1.0, -1.0, 3.3e38, -3.3e38, 1.17549435e-38, np.float32(1) + np.float32(2 ** -23)], np.float32),
         rng.uniform(-1, 1, 5000).astype(np.float32).view(np.uint32).__or__(np.uint32(0x00FFFF)).view(np.float32)]
    return np.concatenate(v)


def test_split_is_exact():
    x = values()
    x1, x2, x3 = split3(x)
    assert np.array_equal((x1.astype(np.float64) + x2 + x3), x.astype(np.float64))
    for p in (x1, x2, x3):                              # every piece is a bf16 value
        assert not (p.view(np.uint32) & 0xFFFF).any()
    assert (np.abs(x2) <= np.abs(x1) * 2.0 ** -8).all() and (np.abs(x3) <= np.abs(x1) * 2.0 ** -16).all()


def test_six_terms_bound_the_product_error():
    rng = np.random.default_rng(6)
    x = values()
    w = rng.permutation(values())
    ok = np.abs(x.astype(np.float64) * w) < 1e30         # (the model's fp64 products: no overflow)
    x, w = x[ok], w[ok]
    x1, x2, x3 = (p.astype(np.float64) for p in split3(x))
    w1, w2, w3 = (p.astype(np.float64) for p in split3(w))
    six = x3 * w1 + x2 * w2 + x1 * w3 + x2 * w1 + x1 * w2 + x1 * w1
    exact = x.astype(np.float64) * w
    err = np.abs(six - exact)
    assert (err <= 2.0 ** -22 * np.abs(exact) + 1e-300).all(), float((err / np.maximum(np.abs(exact), 1e-300)).max())
