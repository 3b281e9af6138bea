"""numpy fp64 reference of the resident calibration (qcnn_calib_begin .. qcnn_calib_read, kernel k_ec_gram_panel): the second
moments G_g[p][q] = sum over live images and output pixels of s_p s_q of a layer's input windows, computed from the layer's
input map in the layout the engine keeps it in — image-minor panels [panel][E][128], element e = (iy*W + ix)*C + ch.

geom: dict(kind="conv", H, W, C, grp, k, stride, pad) for a conv layer, dict(kind="fc", H, W, C) for an FC layer on an
H x W x C map (a later FC layer also names first_fc_hwc, the first FC layer's input dims, for the mistake that reuses its map).
Patch index p = (y*k + x)*Cg + c, channel g*Cg + c, out-of-map taps are zeros, Ho / Wo by the floor rule.  An FC layer has one output pixel and P = H*W*C columns: the FIRST FC layer's column d = (c*H + h)*W + w is element (h*W + w)*C + c
(the reference flattens NCHW), a later FC layer's column d is element d.

``mistake`` builds one deliberately wrong variant (tests/test_calib_cases_cpu.py shows that every one of them changes the
result of some crafted case, so a kernel that made it could not pass)."""
import numpy as np

PANEL = 128
MISTAKES = ("dead_lanes_counted", "taps_not_zeroed", "stride_ignored", "group_offset_dropped", "first_fc_in_nhwc_order",
            "later_fc_flattened", "panel_twice", "last_panel_dropped")


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def patch_len(geom):
    if geom["kind"] == "fc":
        return geom["H"] * geom["W"] * geom["C"]
    return geom["k"] * geom["k"] * (geom["C"] // geom["grp"])


def out_pixels(geom):
    if geom["kind"] == "fc":
        return 1
    return conv_out(geom["H"], geom["k"], geom["stride"], geom["pad"]) * conv_out(geom["W"], geom["k"], geom["stride"], geom["pad"])


def to_panels(x_nhwc, junk=977.5):
    """[n][H][W][C] -> [panels][E][128] float32 with ``junk`` in the dead lanes of the last panel."""
    x = np.asarray(x_nhwc, np.float32)
    n = x.shape[0]
    flat = x.reshape(n, -1)
    panels = (n + PANEL - 1) // PANEL
    out = np.full((panels, flat.shape[1], PANEL), junk, np.float32)
    for p in range(panels):
        part = flat[p * PANEL:(p + 1) * PANEL]
        out[p, :, :len(part)] = part.T
    return out


def _columns(geom, fc_flatten, mistake):
    """Per group and output pixel the element index of every column, -1 = a zero: int array [grp][pixels][P]."""
    H, W, C = geom["H"], geom["W"], geom["C"]
    if geom["kind"] == "fc":
        flat = fc_flatten
        if mistake == "first_fc_in_nhwc_order" and fc_flatten:
            flat = False
        if mistake == "later_fc_flattened" and not fc_flatten:         # the FIRST FC layer's map (geom["first_fc_hwc"]) used again
            fh, fw, fc = geom["first_fc_hwc"]
            first = [(h * fw + w) * fc + c for c in range(fc) for h in range(fh) for w in range(fw)]
            return (np.array(first[:H * W * C], np.int64) % (H * W * C))[None, None, :]
        idx = np.empty(H * W * C, np.int64)
        for c in range(C):
            for h in range(H):
                for w in range(W):
                    d = (c * H + h) * W + w
                    idx[d] = (h * W + w) * C + c if flat else d
        return idx[None, None, :]
    grp, k, stride, pad = geom["grp"], geom["k"], geom["stride"], geom["pad"]
    Cg = C // grp
    Ho, Wo = conv_out(H, k, stride, pad), conv_out(W, k, stride, pad)
    step = 1 if mistake == "stride_ignored" else stride
    idx = np.full((grp, Ho * Wo, k * k * Cg), -1, np.int64)
    for g in range(grp):
        for oy in range(Ho):
            for ox in range(Wo):
                for y in range(k):
                    for x in range(k):
                        iy, ix = oy * step - pad + y, ox * step - pad + x
                        inside = 0 <= iy < H and 0 <= ix < W
                        if not inside:
                            if mistake != "taps_not_zeroed":
                                continue
                            iy, ix = min(max(iy, 0), H - 1), min(max(ix, 0), W - 1)       # the nearest element instead of a zero
                        for c in range(Cg):
                            ch = c if mistake == "group_offset_dropped" else g * Cg + c
                            idx[g, oy * Wo + ox, (y * k + x) * Cg + c] = (iy * W + ix) * C + ch
    return idx


def gram_from_panels(panels, n, geom, fc_flatten=False, mistake=None):
    """(G float64 [grp][P][P], patch rows) from ``panels`` [panels][E][128] holding ``n`` live images."""
    assert mistake is None or mistake in MISTAKES
    panels = np.asarray(panels)
    idx = _columns(geom, fc_flatten, mistake)
    grp, pix, P = idx.shape
    G = np.zeros((grp, P, P), np.float64)
    rows = 0
    order = list(range(panels.shape[0]))
    if mistake == "panel_twice":
        order = order + [order[0]]
    if mistake == "last_panel_dropped":
        order = order[:-1]
    for p in order:
        live = min(PANEL, n - p * PANEL)
        if mistake == "dead_lanes_counted":
            live = PANEL
        X = panels[p, :, :live].astype(np.float64)                 # [E][live]
        for g in range(grp):
            for o in range(pix):
                col = idx[g, o]
                S = np.where((col >= 0)[:, None], X[np.maximum(col, 0)], 0.0)      # [P][live]
                G[g] += S @ S.T
        rows += live * pix
    return G, rows


def abs_gram_from_panels(panels, n, geom, fc_flatten=False):
    """sum |s_p s_q|: the scale of the kernels' error bound."""
    return gram_from_panels(np.abs(np.asarray(panels, np.float64)), n, geom, fc_flatten)[0]


def units_per_split(geom, panels, run=256, max_slab_bytes=128 << 20):
    """(units per split, splits) of qk_ec_gram_panel_units_per_split (csrc/qcnn_ec.hip), restated: a unit is one (panel, output
    pixel) = 128 patch rows, a split is whole fp32 runs of run / 128 units; as many splits as fill 2048 workgroups with the
    shape's upper-triangle 64 x 64 tile pairs, at most one per run, slabs of at most max_slab_bytes in all."""
    P = patch_len(geom)
    grp = geom.get("grp", 1) if geom["kind"] == "conv" else 1
    nt = (P + 63) // 64
    wgs = nt * (nt + 1) // 2 * grp
    per_run = run // PANEL
    units = panels * out_pixels(geom)
    runs = (units + per_run - 1) // per_run
    one = grp * P * P * 8
    want = max(1, 2048 // wgs)
    want = min(want, max(1, max_slab_bytes // one))
    want = max(1, min(want, runs, 65535))
    per = (runs + want - 1) // want * per_run
    return per, max(1, (units + per - 1) // per)
