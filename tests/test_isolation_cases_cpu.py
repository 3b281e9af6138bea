"""CPU tier of the window-isolation cases (tests/isolation_cases.py; tests/test_gpu_isolation.py sends them through the kernels).

  * Safety first: for every new shape the furthest byte an MFMA builder's operand load can reach past the end of the layer's input
    buffer — (dims missing) x the 512-byte row of a dim, from mfma_load's addressing — equals the figure stated in the module and is
    below kSlack, read out of qcnn_engine.h.  A shape that fails here does not run on a GPU.
  * `hit` against an independent restatement: np.isnan of table_probe.dense_expected (float64, plain loops over taps, groups and
    sub-spaces) on the poisoned input, for every plan of every case — groups and ragged FC sub-spaces included; the padded dims
    of a ragged sub-space's code words are ignored by the restatement (NaN there changes nothing).
  * Every single-element poison bites on both sides: it reaches at least one output of its image and leaves at least one
    untouched.  The exceptions are the stated ones: FC layers (the whole image), sm_ct24's last pixel (no window covers it), the
    centre of sm_15_* (all 36 windows), and the tg_* maps of a few pixels, where the count of pixels that reach no output and of
    pixels that reach every output is stated per shape (isolation_cases.TG_PIXELS); the positions a corner / the centre reaches are
    the recorded ones.
  * Family reach of the new shapes, re-derived from the CPU planner library and the launch rules restated in
    test_panel_cases_cpu.py / test_small_cases_cpu.py / test_exact_cases_cpu.py; k_fc_sym8 refuses a ragged layer by its shape rule.
  * The C oracle on ragged FC layers: it gives the float64 sum within the dense bound (recorded: it does not refuse them)."""
import functools
import os
import re
import sys
import traceback

import numpy as np
import pytest

import isolation_cases as ic
import table_probe as tp
from conftest import ROOT, pkg
from test_exact_cases_cpu import slices_of
from test_gpu_table_probe import SLIDE, SPLIT_TILE, TILE, code_ok
from test_panel_cases_cpu import derive, plan
from test_planner_cpu import COSTS, fc_planner, planner          # (fixtures)
from test_small_cases_cpu import chunks_of, constants, conv_small_plan, stage_group
from test_table_probe_cpu import oracle_out

synth = pkg("synth")

CONV_PANEL = sorted(tp.PANEL_REACH) + ic.IG + ic.TG
CONV_FEW = sorted(n for n in tp.SMALL_REACH if tp.SHAPES[n][0] == "conv")
FC_ALL = sorted(ic.ec.FC) + ic.FR + sorted(n for n in tp.SMALL_REACH if tp.SHAPES[n][0] == "fc") + tp.DEC_FC_SHAPES
EVERY = CONV_PANEL + ["rgb7"] + CONV_FEW + FC_ALL


def in_child(fn):
    """Run a test body in a forked child process and fail with its traceback.  The bodies below fill numpy's and the C oracle's
    heap blocks with NaN and free them; the compiled reference, which other tests of this tier load into the same process,
    scales an UNINITIALISED result buffer by beta = 0 before it accumulates (cblas_sgemm_nn: pc[in] *= beta), and 0 * NaN is
    NaN — non-finite garbage left in the heap would surface there as a wrong feature map.  A child's heap dies with it."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        r, w = os.pipe()
        pid = os.fork()
        if pid == 0:
            code = 1
            try:
                os.close(r)
                fn(*args, **kwargs)
                code = 0
            except BaseException:
                os.write(w, traceback.format_exc().encode()[-32768:])
            finally:
                sys.stdout.flush()
                sys.stderr.flush()
                os._exit(code)
        os.close(w)
        text = b""
        while True:
            chunk = os.read(r, 65536)
            if not chunk:
                break
            text += chunk
        os.close(r)
        _, status = os.waitpid(pid, 0)
        assert status == 0, "in the child process (wait status %d):\n%s" % (status, text.decode(errors="replace"))
    return wrapper


def random_params(name, seed=5):
    """Ordinary random parameters of a case's layer (file layout), whatever its D % Cs."""
    kind, g, M, K, Cs = ic.shape_of(name)
    d = g["Cin"] // g["grp"] if kind == "conv" else g["D"]
    spec = {0: dict(kind=kind, M=M, K=K, Cs=Cs, Ct=g["Ct"], knl=g["knl"] if kind == "conv" else 1, D=d)}
    return synth.make_params(None, None, seed=seed, spec=spec)[0]


# ---------------------------------------------------------------- safety: how far the over-read goes ----
def test_over_read_of_the_new_shapes_stays_inside_the_slack():
    src = open(os.path.join(ROOT, "quantized-cnn_amd", "csrc", "qcnn_engine.h")).read()
    m = re.search(r"constexpr size_t kSlack = (\d+) \* (\d+);", src)
    assert m and int(m.group(1)) * int(m.group(2)) == ic.K_SLACK
    rows = re.search(r"\[E_l\]\[128\]", open(os.path.join(ROOT, "quantized-cnn_amd", "csrc", "qcnn_kernels.h")).read())
    assert rows and ic.ROW_BYTES == 128 * 4
    assert sorted(ic.OVER_READ_BYTES) == sorted(ic.SHAPES)
    for name in sorted(ic.SHAPES):
        kind, g, M, K, Cs = ic.shape_of(name)
        o = ic.over_read(kind, g, M, K, Cs)
        d = g["Cin"] // g["grp"] if kind == "conv" else g["D"]
        assert o["missing"] > 0 and M * Cs > d > (M - 1) * Cs, name                 # a ragged last sub-space, and dims are missing
        assert o["bytes"] == o["rows"] * ic.ROW_BYTES == ic.OVER_READ_BYTES[name], (name, o)
        assert 0 < o["bytes"] < ic.K_SLACK, (name, o)
        print("%s: %d rows = %d bytes past the buffer's end (%d dims missing per group), into %s" % (name, o["rows"], o["bytes"], o["missing"], o["into"]))
    # rgb7 read in place (NCHW): dims are channel planes, clamped per lane to the group's last one; the second k-step (Cs = 8) starts
    # at plane 4, so planes 3 .. 6 of the LAST image lie behind the batch: four planes of 31 x 31 floats in the staging buffer's slack
    kind, g, M, K, Cs = ic.shape_of("rgb7")
    assert (g["Cin"], M, Cs) == (3, 1, 8) and (4 + g["Cin"] - g["Cin"]) * g["H"] * g["W"] * 4 < ic.K_SLACK


# ---------------------------------------------------------------- hit against the float64 restatement ----
@pytest.mark.parametrize("name", EVERY)
@in_child
def test_hit_is_where_the_float64_sum_is_nan(name):
    kind, g, M, K, Cs = ic.shape_of(name)
    params = random_params(name)
    few = name in CONV_FEW or name in tp.SMALL_REACH
    masks = []
    if not few or kind == "fc":
        n = 12 if kind == "conv" else 6                  # a plan's elements, folded onto a few images: one element per image still
        p = ic.plan(kind, g, M, Cs)
        for i in range(0, len(p["single"]), n - 1):
            chunk = [(j,) + e[1:] for j, e in enumerate(p["single"][i:i + n - 1])]
            masks.append(ic.mask_of(kind, g, n, chunk, whole=[n - 1]))
    if few or name in ic.FR or name in ic.IG or name in ic.TG:
        for _, e in ic.few_plans(kind, g, M, Cs):
            masks.append(ic.mask_of(kind, g, 3, [(1,) + e], whole=[2]))
    for mask in masks:
        x = ic.poisoned(tp.activations(kind, g, mask.shape[0], seed=6, scaled=False), mask)
        want64, _ = tp.dense_expected(kind, g, x, params)
        h = ic.hit(kind, g, mask)
        assert h.shape == want64.shape and np.array_equal(np.isnan(want64), h), (name, int((np.isnan(want64) != h).sum()))
        assert np.isfinite(want64[~h]).all()


@pytest.mark.parametrize("name", ic.FR + ic.IG + ["pn_partial", "sm_m18"])
@in_child
def test_padded_code_word_dims_are_ignored(name):
    """NaN in the dims a ragged last sub-space does not have (the file layout keeps them; synth.make_params fills them with random
    numbers) changes no bit of the float64 sum: the restatement reads the live dims only."""
    kind, g, M, K, Cs = ic.shape_of(name)
    params = random_params(name)
    cse = tp.cs_eff(kind, g, M, Cs)
    assert cse[-1] < Cs
    x = tp.activations(kind, g, 2, seed=7, scaled=False)
    a, _ = tp.dense_expected(kind, g, x, params)
    ctrd = params["ctrd"].copy()
    ctrd[M - 1, :, cse[-1]:] = np.nan
    b, _ = tp.dense_expected(kind, g, x, dict(params, ctrd=ctrd))
    assert np.isfinite(a).all() and np.array_equal(a, b)


# ---------------------------------------------------------------- every poison bites on both sides ----
def positions(h):
    return h.any(-1).reshape(h.shape[0], -1).sum(1)


@pytest.mark.parametrize("name", EVERY)
def test_every_single_poison_reaches_something_and_not_everything(name):
    kind, g, M, K, Cs = ic.shape_of(name)
    if kind == "fc":                                     # stated exception: an FC output depends on every input dim of its image
        mask, p = ic.plan_mask(kind, g, M, Cs)
        h = ic.hit(kind, g, mask)
        for i, _, _, c in p["single"]:
            assert h[i].all() and 0 <= c < g["D"]
        assert [c for _, _, _, c in p["single"]] == ic.channels(kind, g, M, Cs) and g["D"] - 1 in ic.channels(kind, g, M, Cs)
        assert not h[p["clean"]].any() and h[p["whole"]].all()
        return
    Ho, Wo = tp.out_hw(g)
    if name in CONV_FEW:
        elems = [(1,) + e for _, e in ic.few_plans(kind, g, M, Cs)]
        hs = [(e, ic.hit(kind, g, ic.mask_of(kind, g, 3, [e]))[1]) for e in elems]
    else:
        for n in (ic.BATCH, ic.SPLIT_BATCH):
            mask, p = ic.plan_mask(kind, g, M, Cs, n)
            assert len({e[0] for e in p["single"]}) == len(p["single"]) and not set(p["whole"]) & set(p["clean"])
            assert mask[p["whole"]].all() and not mask[p["clean"]].any() and mask.reshape(n, -1).sum(1).max() == mask[0].size
            assert (mask.reshape(n, -1).sum(1)[[e[0] for e in p["single"]]] == 1).all()
        mask, p = ic.plan_mask(kind, g, M, Cs)
        h = ic.hit(kind, g, mask)
        hs = [(e, h[e[0]]) for e in p["single"]]
        px = {(e[1], e[2]) for e in p["single"]}
        if g["H"] * g["W"] <= 100:
            assert len(px) == g["H"] * g["W"]                                           # one image per input pixel
        assert {(0, 0), (g["H"] - 1, g["W"] - 1)} <= px
        assert {e[3] for e in p["single"]} >= set(ic.channels(kind, g, M, Cs))           # every listed channel is used
        assert any(i < 64 for i, *_ in p["single"]) and any(64 <= i < 126 for i, *_ in p["single"])   # both halves of the panel
    if name in ic.TG:                                    # stated per shape: how many pixels reach no output, how many every output
        by_px = {(e[1], e[2]): (not hi.any(), bool(hi.all())) for e, hi in hs}
        assert all((not hi.any(), bool(hi.all())) == by_px[e[1], e[2]] for e, hi in hs)          # the channel makes no difference
        got = (sum(v[0] for v in by_px.values()), sum(v[1] for v in by_px.values()), len(by_px))
        assert got == ic.TG_PIXELS[name] and got[2] == g["H"] * g["W"], (name, got)
        whole = ic.hit(kind, g, mask)                    # ... and the plan as a whole has NaN and clean outputs side by side
        assert whole.any() and not whole.all() and whole[p["whole"]].all() and not whole[p["clean"]].any()
        hs = []
    for e, hi in hs:
        none, every = not hi.any(), hi.all()
        last_pixel = (e[1], e[2]) == (g["H"] - 1, g["W"] - 1)
        if name in ic.REACHES_NONE and last_pixel:
            assert none, (name, e)
        elif name in ic.REACHES_ALL and (e[1], e[2]) == ic.centre(g) and g["grp"] == 1:
            assert every and int(positions(hi[None])[0]) == Ho * Wo == 36, (name, e)
        else:
            assert not none and not every, (name, e)
    if name in ic.POSITIONS:                             # the recorded counts, from table_probe.window_hit itself
        one = lambda h, w: np.zeros((1, g["H"], g["W"], g["Cin"]), bool)
        m0, m1 = one(0, 0), one(0, 0)
        m0[0, 0, 0, 0] = True
        m1[(0,) + ic.centre(g) + (0,)] = True
        assert (int(tp.window_hit(g, m0).sum()), int(tp.window_hit(g, m1).sum()), Ho * Wo) == ic.POSITIONS[name], name
        assert int(positions(ic.hit(kind, g, m0))[0]) == ic.POSITIONS[name][0]
    if g["grp"] > 1:                                     # a group's poison leaves the other group alone
        Cg, Ctg = g["Cin"] // g["grp"], g["Ct"] // g["grp"]
        for e, hi in hs:
            q = e[3] // Cg
            assert hi[..., q * Ctg:(q + 1) * Ctg].any() and not np.delete(hi, np.s_[q * Ctg:(q + 1) * Ctg], axis=-1).any()


def test_stated_exceptions():
    assert sorted(ic.POSITIONS) == sorted(CONV_PANEL)
    g = tp.SHAPES["sm_ct24"][1]
    m = ic.mask_of("conv", g, 1, [(0, g["H"] - 1, g["W"] - 1, g["Cin"] - 1)])
    assert not ic.hit("conv", g, m).any() and (g["W"] - 1) % g["stride"] == 1
    for n in ic.REACHES_ALL:
        g = tp.SHAPES[n][1]
        m = ic.mask_of("conv", g, 1, [(0,) + ic.centre(g) + (0,)])
        assert ic.hit("conv", g, m).all() and tp.out_hw(g) == (6, 6)


# ---------------------------------------------------------------- what the new shapes reach ----
@pytest.mark.parametrize("name", ic.IG)
def test_new_conv_shapes_reach_their_families(name, planner):
    shape = ic.SHAPES[name]
    kind, g, M, K, Cs, _ = shape
    reach = ic.IG_REACH[name]
    d = derive(shape)
    assert (d["G"], d["last_group"], d["per_pixel"]) == reach["stage"]
    whole = [k for k in reach["live"] if k != "split_tile"]
    assert sorted(k for k in COSTS if k in d) == sorted(whole)                           # no family beyond the listed ones
    for k in whole:
        assert d[k] == reach["live"][k], (name, k, d[k])
    fams = {"tile": TILE, "slide16": SLIDE}
    for panels in (1, 2):                                # 131 images, and the stale run's batches of 70, 5 and 3
        for k in whole:
            costs, ch = plan(planner, shape, panels, fams[k]["opts"])
            assert costs[k] > 0.0 and code_ok(fams[k]["code"], (ch["family"], len(ch["segs"]) - 1 if ch["segs"] else ch["Z"])), (name, k, ch)
            if k == "slide16":
                assert ch["segs"] == reach["segs"]
            else:
                assert ch["Z"] <= 1
        on = dict(TILE["opts"], split=1, slide=1, sym=1, sym8=1, half8=1)
        costs, _ = plan(planner, shape, panels, on)
        assert all(costs[k] == 0.0 for k in COSTS if k not in whole), (name, costs)      # an incomplete sub-space: no eight-wave form
    _, ch = plan(planner, shape, 1, SPLIT_TILE["opts"])
    if "split_tile" in reach["live"]:
        assert (ch["family"], ch["Z"], ch["split_from"]) == (-1,) + reach["live"]["split_tile"] and ch["Z"] > 1
    else:
        assert ch["Z"] <= 1
    p = conv_small_plan(g, M, K, Cs, constants())
    assert p is not None and (p["TH"], p["TW"], p["MC"], p["CH"], p["chunks"], stage_group(K)) == reach["small"]
    cse = tp.cs_eff(kind, g, M, Cs)
    assert g["grp"] == 2 and cse[-1] < Cs and K in (32, 128)


def test_what_the_new_conv_shapes_are_there_for():
    R = ic.IG_REACH
    assert tp.cs_eff(*ic.SHAPES["ig_grp2_ragged"][:2], 3, 8) == [8, 8, 4] and set(R["ig_grp2_ragged"]["live"]) == {"tile", "slide16", "split_tile"}
    assert tp.cs_eff(*ic.SHAPES["ig_grp2_cs4_k32"][:2], 4, 4) == [4, 4, 4, 2] and R["ig_grp2_cs4_k32"]["stage"] == (4, 4, 1)   # ONE stage per pixel:
    assert tp.cs_eff(*ic.SHAPES["ig_grp2_cs4_m5"][:2], 5, 4) == [4, 4, 4, 4, 2]                                              # kept code-book operands
    assert R["ig_grp2_cs4_m5"]["stage"] == (4, 1, 2)                                    # a last stage of one sub-space, three past the end


@pytest.mark.parametrize("name", ic.FR)
def test_new_fc_shapes_reach_their_families(name, fc_planner):
    kind, g, M, K, Cs = ic.shape_of(name)
    reach = ic.FR_REACH[name]
    G = stage_group(K)
    stages = -(-M // G)
    assert reach["G"] == G and g["D"] % Cs == 2 and M * Cs - g["D"] == 2
    geom = [g["D"], g["Ct"], M, K, Cs, 1]
    for key, split, batches in (("plain", 0, ((2, 128), (2, 3), (1, 128), (1, 70), (1, 5), (1, 3))), ("split", 1, ((1, ic.SPLIT_BATCH),))):
        fam, z, per, last = reach[key]
        for panels, live in batches:
            for lut in (1, 2, 3):
                for sym8 in (0, 2):                       # forcing the eight-wave form changes nothing: D != 4 M is refused by its shape rule
                    assert fc_planner(geom + [panels, live], split=split, sym8=sym8, decode=0, lut=lut) == (fam, z), (name, key, lut, sym8)
        assert fam == -1 and slices_of(stages, z) == (per, last) and (z - 1) * per < stages and z > 1
        assert fc_planner(geom + [2, 128], split=split, sym8=0, decode=0, lut=0) == (-1, 1)
    # the shape it is derived from differs in D alone, and reaches the same slices where it runs the same kernel
    src = ic.FR_FROM[name]
    k2, g2, M2, K2, Cs2 = ic.shape_of(src)
    assert (g2["D"] - 2, g2["Ct"], M2, K2, Cs2) == (g["D"], g["Ct"], M, K, Cs)
    if src in ic.ec.FA:
        assert ic.ec.EXACT_REACH[src]["plain"] == reach["plain"] and ic.ec.EXACT_REACH[src]["split"] == reach["split"]
    c = constants()
    MC = min(M, c["LUT_BYTES"] // (K * 4))
    assert K % 4 == 0 and (MC, G) == reach["small"]
    if src in tp.SMALL_REACH:
        assert tp.SMALL_REACH[src] == reach["small"] and chunks_of(M, MC) == [224, 6]


def test_the_eight_wave_fc_kernel_refuses_a_ragged_layer(fc_planner):
    """fx_slices runs k_fc_sym8 (code -5) under QCNN_OPT_SYM8 = 2; the same layer with two input dims less keeps k_fc_aprx: the shape
    rule D == 4 M (qk_fc_sym8_shape) is the refusal, in front of every launch."""
    g, M, K, Cs = ic.ec.FC["fx_slices"][:4]
    assert fc_planner([g["D"], g["Ct"], M, K, Cs, 1, 2, 128], split=0, sym8=2, decode=0, lut=1)[0] == -5
    assert fc_planner([g["D"] - 2, g["Ct"], M, K, Cs, 1, 2, 128], split=0, sym8=2, decode=0, lut=1)[0] == -1


# ---------------------------------------------------------------- the oracle on ragged FC layers ----
@pytest.mark.parametrize("name", ic.FR)
@in_child
def test_oracle_takes_a_ragged_fc_layer(name):
    """Recorded: the C oracle does not refuse M Cs > D; its output stays inside the dense-sum bound against the float64 sum, and NaN in
    the padded code-word dims does not reach it."""
    kind, g, M, K, Cs = ic.shape_of(name)
    params = random_params(name)
    x = tp.activations(kind, g, 3, seed=8, scaled=False)
    want64, mag = tp.dense_expected(kind, g, x, params)
    y = oracle_out(kind, g, params, x)
    worst = tp.dense_check(y, want64, mag, tp.dense_count(kind, g, M, Cs), what=name)
    ctrd = params["ctrd"].copy()
    ctrd[M - 1, :, tp.cs_eff(kind, g, M, Cs)[-1]:] = np.nan
    assert np.array_equal(oracle_out(kind, g, dict(params, ctrd=ctrd), x), y)
    print("%s: oracle worst err / bound %.3f" % (name, worst))
    assert worst <= 1.0
