"""CPU tier of the large-map cases (tests/test_gpu_large_cases.py, the lg_* shapes of tests/table_probe.py): feature maps whose
panel — H W C rows of 128 images, 512 bytes each — reaches beyond 2^31 and beyond 2^32 bytes.

  * Offset arithmetic, in Python integers: per shape the largest source and destination byte offset inside a panel and its side
    of 2^31 and 2^32; the exact set of output rows a source-pixel offset WRAPPED modulo 2^32 changes, and the set a 32-bit
    offset SIGN-EXTENDED at 2^31 changes.  lg_in_lo: no wrapped row, 64 sign-extended ones; lg_in_hi / lg_in_hi_g2: the wrap
    changes output rows 127 .. 131 and no other; lg_dec_lo lies below the decoded panel form's 2^31-byte guard, lg_dec_hi above.
  * Reach: LARGE_REACH is re-derived from the launchers' rules and the planner library (one panel: the three images of the GPU
    tier), as tests/test_tiny_cases_cpu.py does for TINY_REACH; every family that forms a source pixel's byte offset is live on
    lg_in_hi, and the planner cuts no tile of these shapes (no split form, no k_conv_sum launch).
  * Reference: table_probe.dense_expected_by_taps — float64, knl^2 matrix products per group over the decoded weights — is held
    to dense_expected on three pn_* shapes (two groups, stride 2, a ragged last sub-space) within n 2^-53 mag, n = Cg knl^2 + 1
    the terms of a sum: the same exact products in another order.  (Each sum lies within (n - 1) 2^-53 mag of the exact value;
    their distance is printed.)
  * Teeth, on one image: a float32 tap-by-tap sum meets gamma(knl^2 M + CsEff + 1) mag on lg_in_hi; over an input whose source
    rows >= 128 are replaced by rows - 128 — what a wrap modulo 2^32 reads — it leaves the bound at every output position of rows
    127 .. 131 and at no element of any other row; over an input whose rows >= 64 hold unrelated data — lg_in_lo's sign-extension
    pattern: the offset points in front of the panel — it leaves it in rows 63 .. 126.  "At every position": a single element
    whose third of replaced terms happens to sum to the right value within 3.5e-5 of mag has probability about 1.5e-3, so the
    assertion is on positions (at least nine tenths of a position's 128 channels leave the bound), not on all 82 000 elements.
  * The library as it stands forms the source-pixel offset in 32 bits: what this tier shows for lg_in_hi / lg_in_hi_g2 is what the
    conv table kernels return on them (LABBOOK.md, "Large maps"), and the GPU tier does not send those two shapes through them."""
import numpy as np
import pytest

import table_probe as tp
from conftest import pkg
from test_decoded_cases_cpu import conv_dec_instance, conv_dec_shape
from test_gpu_table_probe import EXACT, SPLIT_SYM8, SPLIT_TILE, TILE, code_ok
from test_panel_cases_cpu import FAMS, derive, plan
from test_planner_cpu import COSTS, planner          # (the fixture)
from test_small_cases_cpu import LDS_PER_WORKGROUP, constants, conv_small_plan, stage_group

synth = pkg("synth")

LARGE = sorted(tp.LARGE_SHAPES)
B31, B32 = 1 << 31, 1 << 32
ROW = 512                                  # bytes of one (pixel, channel) row of a panel: 128 images x 4


# ---------------------------------------------------------------- offset arithmetic ----
def pixel_offsets(g):
    """int offsets [H, W] (Python integers in an object array would be slow: int64 holds them) of every source pixel inside its
    panel: (hi W + wi) Cin 512 — pixel_off of qcnn_dev.h in exact arithmetic."""
    hi, wi = np.arange(g["H"], dtype=np.int64)[:, None], np.arange(g["W"], dtype=np.int64)[None, :]
    return (hi * g["W"] + wi) * (g["Cin"] * ROW)


def rows_reading(g, bad):
    """bad [H, W] bool -> the sorted output rows whose window holds a bad source pixel."""
    hit = tp.window_hit(g, bad[None, :, :, None])[0]
    return [int(r) for r in np.nonzero(hit.any(1))[0]]


def offsets_of(name):
    kind, g, M, K, Cs, _ = tp.LARGE_SHAPES[name]
    Ho, Wo = tp.out_hw(g)
    off = pixel_offsets(g)
    src_max = int(off.max()) + g["Cin"] * ROW - 1                # last byte of the last pixel's last channel row
    dst_max = tp.panel_bytes(Ho, Wo, g["Ct"]) - 1
    assert src_max == tp.panel_bytes(g["H"], g["W"], g["Cin"]) - 1
    wrapped = rows_reading(g, off >= B32)                        # a 32-bit product: the pixel at off mod 2^32 is read instead
    signed = rows_reading(g, (off % B32) >= B31)                 # a 32-bit offset sign-extended: a pixel in front of the panel
    return dict(src_max=src_max, dst_max=dst_max, wrapped=wrapped, signed=signed, Ho=Ho)


def test_offsets_of_every_shape():
    o = {n: offsets_of(n) for n in LARGE}
    for n in LARGE:
        print("%s: largest source offset %d, largest destination offset %d; rows a wrap changes %s, rows a sign extension changes %s"
              % (n, o[n]["src_max"], o[n]["dst_max"], span_text(o[n]["wrapped"]), span_text(o[n]["signed"])))
    # the panel sizes the shapes are there for
    assert o["lg_in_lo"]["src_max"] + 1 == 4261412864 and B31 < o["lg_in_lo"]["src_max"] < B32
    assert o["lg_in_hi"]["src_max"] + 1 == 4429185024 == o["lg_in_hi_g2"]["src_max"] + 1 and o["lg_in_hi"]["src_max"] >= B32
    assert o["lg_out"]["dst_max"] + 1 == 4429185024 and o["lg_out"]["src_max"] < B31
    assert o["lg_dec_lo"]["src_max"] + 1 == 2145982464 < B31 <= 2149615104 == o["lg_dec_hi"]["src_max"] + 1
    assert all(o[n]["dst_max"] < B31 for n in LARGE if n != "lg_out")
    # lo: nothing wraps, the lower half of the map is beyond 2^31 (source rows 64 .. 126: output rows 63 .. 126)
    assert o["lg_in_lo"]["wrapped"] == [] and o["lg_in_lo"]["signed"] == list(range(63, 127))
    # hi: source rows 128 .. 131 start at 2^32 exactly (128 x 128 pixels x 512 channels x 512 bytes); output rows 127 .. 131
    for n in ("lg_in_hi", "lg_in_hi_g2"):
        assert o[n]["wrapped"] == [127, 128, 129, 130, 131] and o[n]["Ho"] == 132
        assert o[n]["signed"] == list(range(63, 129))            # offsets in [2^31, 2^32): source rows 64 .. 127 (rows 128 .. wrap to < 2^31)
    g = tp.LARGE_SHAPES["lg_in_hi"][1]
    assert int(pixel_offsets(g)[128, 0]) == B32 and int(pixel_offsets(g)[64, 0]) == B31
    # the group's channel offset comes on top: the last byte the second group reads
    g2 = tp.LARGE_SHAPES["lg_in_hi_g2"][1]
    assert g2["grp"] == 2 and int(pixel_offsets(g2)[131, 127]) + (g2["Cin"] // 2) * ROW >= B32
    # a small input; the decoded shapes either side of 2^31
    assert o["lg_out"]["wrapped"] == o["lg_out"]["signed"] == []
    assert o["lg_dec_lo"]["wrapped"] == o["lg_dec_lo"]["signed"] == [] == o["lg_dec_hi"]["wrapped"]
    assert o["lg_dec_hi"]["signed"] == [147] and o["lg_dec_hi"]["Ho"] == 148      # the last window row reads source rows 1176 .. 1182
    # the glue map; the shapes the 32-bit offset wraps on
    assert tp.panel_bytes(*tp.LARGE_GLUE_MAP) == 4429185024
    assert sorted(n for n in LARGE if o[n]["wrapped"]) == sorted(tp.LARGE_WRAPPING)


def span_text(rows):
    return "none" if not rows else "%d .. %d (%d)" % (rows[0], rows[-1], len(rows))


def test_the_decoded_guard_lies_between_the_two_decoded_shapes():
    """qk_conv_dec refuses an input panel of 2^31 bytes or more (signed 32-bit byte offsets); launch_conv then runs the table kernel."""
    for n, below in (("lg_dec_lo", True), ("lg_dec_hi", False)):
        kind, g, M, K, Cs, _ = tp.LARGE_SHAPES[n]
        assert conv_dec_shape(g, M) is not None                  # the shape decodes; only the size decides
        assert (tp.panel_bytes(g["H"], g["W"], g["Cin"]) < B31) == below


# ---------------------------------------------------------------- reach ----
@pytest.mark.parametrize("name", LARGE)
def test_every_listed_family_is_live_and_nothing_is_cut(name, planner):
    shape = tp.LARGE_SHAPES[name]
    kind, g, M, K, Cs, _ = shape
    reach = tp.LARGE_REACH[name]
    d = derive(shape)
    assert (d["G"], d["last_group"], d["per_pixel"]) == reach["stage"], (name, d)
    assert not [k for k in reach["live"] if k.startswith("split_")]
    for k in reach["live"]:
        assert d.get(k) == reach["live"][k], (name, k, d.get(k))
    assert sorted(k for k in COSTS if k in d) == sorted(reach["live"]), (name, sorted(d))
    assert set(reach["dead"]) == set(COSTS) - set(reach["live"])
    Ho, Wo = tp.out_hw(g)
    for k in COSTS:                                          # one panel: three images
        costs, ch = plan(planner, shape, 1, FAMS[k]["opts"])
        got = (ch["family"], len(ch["segs"]) - 1 if ch["segs"] else ch["Z"])
        if k in reach["live"]:
            assert costs[k] > 0.0 and code_ok(FAMS[k]["code"], got) and ch["Z"] <= 1, (name, k, ch)
            if "slide" in k:
                assert ch["segs"][0] == 0 and ch["segs"][-1] == Ho and len(ch["segs"]) >= 2, (name, k, ch)
        else:
            assert costs[k] == 0.0, (name, k, costs)
    _, ch = plan(planner, shape, 1, EXACT["opts"])
    assert ch["family"] == -1 and ch["Z"] <= 1
    for f in (SPLIT_TILE, SPLIT_SYM8):                       # thousands of tiles fill the chip: QCNN_OPT_SPLIT cuts nothing
        _, ch = plan(planner, shape, 1, f["opts"])
        assert ch["Z"] <= 1, (name, f["label"], ch)
    p = conv_small_plan(g, M, K, Cs, constants())
    assert p is not None and (p["TH"], p["TW"], p["MC"], p["CH"], p["chunks"], stage_group(K)) == reach["small"], (name, p)
    assert p["lds"] <= LDS_PER_WORKGROUP
    if "dec" in reach:
        kp, s = conv_dec_shape(g, M)
        ns = kp // 4
        many = conv_dec_instance(g, 128, 2)
        assert (s, ns, g["knl"] * ns, many, conv_dec_instance(g, tp.LARGE_BATCH, 1), g["Ct"] // (16 * many[0])) == reach["dec"]
    else:
        assert conv_dec_shape(g, M) is None


def test_what_each_shape_is_there_for():
    S, R = tp.LARGE_SHAPES, tp.LARGE_REACH
    assert sorted(S) == sorted(R)
    # every family that reads through pixel_off is live where source offsets pass 2^32 (the exact builder is the tile kernel
    # under QCNN_LUT_EXACT: always eligible)
    assert set(R["lg_in_hi"]["live"]) == set(COSTS) == set(R["lg_in_lo"]["live"])
    assert set(R["lg_in_hi_g2"]["live"]) == {"tile", "slide16"} and S["lg_in_hi_g2"][1]["grp"] == 2
    assert S["lg_in_hi_g2"][1] == dict(S["lg_in_hi"][1], grp=2) and S["lg_in_hi"][1] == dict(S["lg_in_lo"][1], H=132)
    # output stores beyond 2^32 through the tile, sliding, eight-wave sliding and both half-panel forms
    assert set(R["lg_out"]["live"]) == {"tile", "slide16", "sym8_slide", "half8", "half8_slide"}
    for n in ("lg_dec_lo", "lg_dec_hi"):
        assert S[n][1]["Cin"] == 3 and S[n][2] == 1 and set(R[n]["live"]) == {"tile"} and not R[n]["dec"][3][2]     # unpadded: no clamps
    for n in LARGE:                                          # dense sums: one missing term stays visible (2^24 / terms^2 bounds)
        assert S[n][1]["knl"] ** 2 * S[n][2] <= 1200


# ---------------------------------------------------------------- the tap-by-tap reference ----
@pytest.mark.parametrize("name", ["pn_grp2_5x5", "pn_s2_5x5", "pn_partial"])
def test_tap_by_tap_reference_is_dense_expected_in_another_order(name):
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    spec = {0: dict(kind=kind, M=M, K=K, Cs=Cs, Ct=g["Ct"], knl=g["knl"], D=g["Cin"] // g["grp"])}
    params = synth.make_params(None, None, seed=201, spec=spec)[0]
    x = tp.activations(kind, g, 3, seed=202, scaled=False)
    want64, mag = tp.dense_expected(kind, g, x, params)
    got64, gmag = tp.dense_expected_by_taps(g, x, params)
    n = g["Cin"] // g["grp"] * g["knl"] ** 2 + 1
    ratio = np.abs(got64 - want64) / (n * 2.0 ** -53 * mag)
    mratio = np.abs(gmag - mag) / (n * 2.0 ** -53 * mag)
    print("%s: tap-by-tap against dense_expected: worst |d want| / (n 2^-53 mag) = %.3f, |d mag| = %.3f (n = %d)" % (name, ratio.max(), mratio.max(), n))
    assert ratio.max() <= 1.0 and mratio.max() <= 1.0
    Ho, _ = tp.out_hw(g)
    part, pmag = tp.dense_expected_by_taps(g, x, params, rows=(Ho - 3, Ho))      # a crop of output rows: the same numbers
    assert np.array_equal(part, got64[:, Ho - 3:]) and np.array_equal(pmag, gmag[:, Ho - 3:])


# ---------------------------------------------------------------- teeth, on one image ----
def sum32_by_taps(g, x, params):
    """The layer in float32, tap by tap: bias + knl^2 float32 matrix products per group over the decoded weights.  At most
    Cg + knl^2 roundings behind any term, whatever order the matrix product sums in: inside gamma(knl^2 M + CsEff + 1) wherever
    Cg + knl^2 + 1 <= knl^2 M + CsEff + 1."""
    x = np.asarray(x, np.float32)
    n, H, W, Cin = x.shape
    knl, s, pad, grp, Ct = g["knl"], g["stride"], g["pad"], g["grp"], g["Ct"]
    ctrd = np.asarray(params["ctrd"], np.float32)
    M, K, Cs = ctrd.shape
    Ho, Wo = tp.out_hw(g)
    Cg, Ctg = Cin // grp, Ct // grp
    a = np.asarray(params["asmt"]).reshape(Ct, knl, knl, M).astype(np.int64)
    w = ctrd[np.arange(M)[None, None, None, :], a].reshape(Ct, knl, knl, M * Cs)[..., :Cg]
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, Cin), np.float32)
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.tile(np.asarray(params["bias"], np.float32), (n, Ho, Wo, 1))
    for gi in range(grp):
        cts, cin = slice(gi * Ctg, (gi + 1) * Ctg), slice(gi * Cg, (gi + 1) * Cg)
        for kh in range(knl):
            for kw in range(knl):
                y[..., cts] += np.ascontiguousarray(xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, cin]) @ w[cts, kh, kw].T
    return y


def one_image_case(name, seed):
    kind, g, M, K, Cs, _ = tp.LARGE_SHAPES[name]
    spec = {0: dict(kind=kind, M=M, K=K, Cs=Cs, Ct=g["Ct"], knl=g["knl"], D=g["Cin"] // g["grp"])}
    params = synth.make_params(None, None, seed=seed, spec=spec)[0]
    x = tp.activations(kind, g, 1, seed=seed + 1, scaled=False)
    want64, mag = tp.dense_expected_by_taps(g, x, params)
    n_terms = tp.dense_count(kind, g, M, Cs)
    assert g["Cin"] // g["grp"] + g["knl"] ** 2 + 1 <= n_terms
    return g, params, x, want64, mag, n_terms


def rows_beyond(y, want64, mag, n_terms):
    """(share of elements beyond the bound per output row [Ho], least share over a row's positions [Ho])."""
    bad = np.abs(y.astype(np.float64) - want64) > tp.gamma(n_terms) * mag
    return bad[0].mean(axis=(1, 2)), bad[0].mean(axis=2).min(axis=1)


def test_a_wrapped_source_offset_leaves_the_bound_in_rows_127_to_131():
    g, params, x, want64, mag, n_terms = one_image_case("lg_in_hi", 203)
    worst = tp.dense_check(sum32_by_taps(g, x, params), want64, mag, n_terms, what="lg_in_hi float32 tap-by-tap sum")
    print("lg_in_hi: float32 tap-by-tap sum worst err / bound %.3f" % worst)
    assert worst <= 1.0
    wrap = x.copy()
    wrap[:, 128:] = x[:, :4]                                 # rows 128 .. 131 read rows 0 .. 3: their offsets modulo 2^32
    share, least = rows_beyond(sum32_by_taps(g, wrap, params), want64, mag, n_terms)
    changed = offsets_of("lg_in_hi")["wrapped"]
    assert changed == [127, 128, 129, 130, 131]
    print("lg_in_hi, wrapped: share of elements beyond the bound in rows 127 .. 131: %s" % np.round(share[127:], 4))
    assert (least[changed] >= 0.9).all(), least[changed]     # every position of those rows ...
    assert (share[:127] == 0).all()                          # ... and no element of any other row


def test_a_sign_extended_source_offset_leaves_the_bound_in_rows_63_to_126():
    g, params, x, want64, mag, n_terms = one_image_case("lg_in_lo", 205)
    assert tp.dense_check(sum32_by_taps(g, x, params), want64, mag, n_terms, what="lg_in_lo float32 tap-by-tap sum") <= 1.0
    other = tp.activations("conv", g, 1, seed=207, scaled=False)
    front = x.copy()
    front[:, 64:] = other[:, 64:]                            # offsets >= 2^31 point in front of the panel: unrelated data
    share, least = rows_beyond(sum32_by_taps(g, front, params), want64, mag, n_terms)
    changed = offsets_of("lg_in_lo")["signed"]
    assert changed == list(range(63, 127))
    assert (least[changed] >= 0.9).all(), least[changed]
    assert (share[:63] == 0).all()
