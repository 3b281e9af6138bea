#!/usr/bin/env python3
"""Device time of the pack step and of the whole call when the source images are read in place under another layout (LABBOOK.md,
"Source layouts"): qcnn_forward_u8_resized_views_strided against qcnn_forward_u8_resized_views, on the rig of
scripts/resize_time.py — 1000 batch slots as 100 images x ten-crop and as 1000 images x the centre view, sources of 256 x 256
and of 500 x 375, full image 256 x 256 with a mean image.

  (a) planar          qcnn_forward_u8_resized_views on planar [C][h][w] images
  (b) strided planar  the strided call on the same bytes under planar descriptors: what the descriptor itself costs
  (c) bgr             interleaved [h][w][3], tight
  (d) bmp24           whole 24-bit BMP files back to back, bottom-up, rows padded to 4 bytes, described by qcnn_src_bmp
  (e) bgra_pitched    4 bytes a pixel, row pitch 64 bytes beyond 4 * w

  pack step    a glue-only model ([relu]) of AlexNet's input shape, no output asked for: a call is the descriptor upload, the
               pack kernel and one ReLU sweep, HIP events around it.
  whole call   AlexNet with synthetic parameters, the fast path, prob + top-5: from BMP files' bytes against from planar bytes.
  host         single-thread numpy time to de-interleave and flip the same files into planar images: the work the strided
               call removes from the host (a CPU figure for context, no bar).

Every layout holds the same samples; before anything is timed fm[0] of the first slots must have the same bits under all five.
Variants alternate inside one process after warm-up, every timed call behind an un-timed one of its kind; median, minimum,
maximum, ratio to (a).
usage: layout_time.py [rounds=20] [--rows=abcde] [--pack-only] [--no-check]
  --rows=a     rows (a) alone, through nothing this script's commit added: what is run at the parent commit for the bar on (a)
  --rows=ab    (a) and (b): the rows a timing-only build of the strided kernels is compared in (QCNN_HIP_LIB names the library;
               -DQK_STRIDED_VAR, quantized-cnn_amd/csrc/qcnn_glue.hip; the bit check then covers planar descriptors alone)
  --pack-only  the pack step alone
  --no-check   go on where the bits differ (a timing-only build without the channel select)"""
import importlib, os, struct, sys, time
import numpy as np
import torch   # before libqcnn_hip.so: both must bind to the HIP runtime torch ships
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n: importlib.import_module("quantized-cnn_amd." + n)

FULL = (256, 256)
SLOTS = 1000
SIZES = ((256, 256), (500, 375))


def timed(stream, calls, rounds, warm=3):
    """{name: [ms]} of the calls, alternating, HIP events on the context's stream around each."""
    for _ in range(warm):
        for _, call in calls:
            call()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in calls}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(rounds):
        for name, call in calls:
            call()                 # un-timed: keeps the device busy while the host prepares the timed call behind it
            ev[0].record(stream)
            call()
            ev[1].record(stream)
            ev[1].synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    return ms


def report(title, ms, yardstick_of):
    print(title)
    for name, v in ms.items():
        base = float(np.median(ms[yardstick_of(name)]))
        print("  %-62s median %.3f ms  min %.3f ms  max %.3f ms  x %.3f of (a)" % (name, float(np.median(v)), min(v), max(v), float(np.median(v)) / base))


def bmp_header(h, w):
    stride = (3 * w + 3) & ~3
    return struct.pack("<2sIHHI", b"BM", 54 + h * stride, 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, h * stride, 2835, 2835, 0, 0)


def layouts_on_device(engine, px):
    """px uint8 [n][3][h][w] on the device -> {layout: (device buffer, [SrcPixels])}, every buffer holding px's samples."""
    n, c, h, w = px.shape
    hwc = px.permute(0, 2, 3, 1).contiguous()                       # [n][h][w][3]
    out = {"strided planar": (px, [engine.src_planar(i * c * h * w, h, w, c) for i in range(n)]),
           "bgr": (hwc, [engine.SrcPixels(i * 3 * h * w, 3 * w, h, w, 3, (0, 1, 2, 0)) for i in range(n)])}
    stride = (3 * w + 3) & ~3
    head = bmp_header(h, w)
    files = torch.zeros((n, 54 + h * stride), dtype=torch.uint8, device=px.device)
    files[:, :54] = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(px.device)
    files[:, 54:].view(n, h, stride)[:, :, :3 * w] = hwc.flip(1).reshape(n, h, 3 * w)          # bottom-up
    d = engine.src_bmp(head + bytes(h * stride), 0)
    out["bmp24"] = (files, [d._replace(offset=d.offset + i * (54 + h * stride)) for i in range(n)])
    pitch = 4 * w + 64
    frames = torch.randint(0, 256, (n, h, pitch), dtype=torch.uint8, device=px.device)
    frames[:, :, :4 * w].view(n, h, w, 4)[..., :3] = hwc
    out["bgra_pitched"] = (frames, [engine.SrcPixels(i * h * pitch, pitch, h, w, 4, (0, 1, 2, 0)) for i in range(n)])
    return out


def host_deinterleave(files, h, w):
    """What a caller of the planar call does on the host: every file's pixel array -> planar [3][h][w], top row first."""
    stride = (3 * w + 3) & ~3
    out = np.empty((len(files), 3, h, w), np.uint8)
    t0 = time.perf_counter()
    for i, f in enumerate(files):
        rows = f[54:].reshape(h, stride)[:, :3 * w].reshape(h, w, 3)
        out[i] = rows[::-1].transpose(2, 0, 1)
    return (time.perf_counter() - t0) / len(files), out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows = ([a[7:] for a in sys.argv[1:] if a.startswith("--rows=")] or ["abcde"])[0]
    planar_only, pack_only = rows == "a", "--pack-only" in sys.argv
    rounds = int(args[0]) if args else 20
    capi, topo, synth, engine = pkg("capi"), pkg("topology"), pkg("synth"), pkg("engine")
    in_chw, layers, _, _ = topo.MODELS["AlexNet"]
    c, h, w = in_chw
    rng = np.random.default_rng(9)
    mean = torch.from_numpy((rng.standard_normal((c,) + FULL) * 20 + 110).astype(np.float32)).cuda()
    ten = engine.ten_crop_views(FULL[0], FULL[1], h, w)
    centre = [ten[4]]
    torch.set_num_threads(1)
    np_threads = os.environ.get("OMP_NUM_THREADS")
    planar, strided = {}, {}
    for hs, ws in SIZES:
        px = torch.from_numpy(rng.integers(0, 256, (SLOTS, c, hs, ws), dtype=np.uint8)).cuda()
        planar[(hs, ws)] = (px, {n: (capi.QcnnSrcImage * n)(*[capi.QcnnSrcImage(i * c * hs * ws, hs, ws) for i in range(n)]) for n in (SLOTS // 10, SLOTS)})
        if not planar_only:
            strided[(hs, ws)] = {name: (buf, {n: engine._pixels_array(descs[:n])[0] for n in (SLOTS // 10, SLOTS)})
                                 for name, (buf, descs) in layouts_on_device(engine, px).items()}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    shapes = ((SLOTS // 10, ten, "%d x ten-crop" % (SLOTS // 10)), (SLOTS, centre, "%d x centre" % SLOTS))
    letter = {name: l for name, l in (("strided planar", "b"), ("bgr", "c"), ("bmp24", "d"), ("bgra_pitched", "e")) if l in rows}

    def variants(eng, outs, which):
        calls = []
        for n, views, label in shapes:
            for (hs, ws) in SIZES:
                px, descs = planar[(hs, ws)]
                tag = "%dx%d  %s" % (hs, ws, label)
                calls.append(("(a) planar          " + tag, lambda n=n, views=views, px=px, descs=descs: eng.forward_u8_resized_views_dev(
                    px.data_ptr(), px.numel(), descs[n], FULL[0], FULL[1], mean.data_ptr(), views, *outs)))
                for name in which:
                    buf, sd = strided[(hs, ws)][name]
                    calls.append(("(%s) %-15s " % (letter[name], name) + tag, lambda n=n, views=views, buf=buf, sd=sd: eng.forward_u8_resized_views_strided_dev(
                        buf.data_ptr(), buf.numel(), sd[n], FULL[0], FULL[1], mean.data_ptr(), views, *outs)))
        return calls

    yardstick_of = lambda name: "(a) planar          " + name[20:]

    # ---- the pack step: glue-only model, no outputs
    glue = engine.QcnnEngine(0, stream=stream.cuda_stream)
    glue.set_option(capi.OPT_KEEP_ALL, 1)
    glue.load_model(in_chw, [topo.relu()], {}, SLOTS)
    calls = variants(glue, (None, None, None), [] if planar_only else list(letter))
    want = {}
    for name, call in calls:                                        # the same samples under every layout: the same bits
        call()
        glue.sync()
        got = glue.layer_output_range(0, 0, 16).view(np.uint32)
        ref = want.setdefault(name[20:], got)
        if not np.array_equal(ref, got):
            print("fm[0] under %s differs from the planar call's" % name)
            if "--no-check" not in sys.argv:
                sys.exit(1)
            want[None] = True
    if None not in want:
        print("fm[0] of the first 16 slots: the same bits under every layout, source size and slot shape")
    report("pack kernel + one ReLU sweep over %d x %d floats (glue-only model), %d rounds:" % (SLOTS, c * h * w, rounds),
           timed(stream, calls, rounds), yardstick_of)
    glue.close()
    if pack_only:
        return

    # ---- the whole call: AlexNet, from planar bytes and from BMP files' bytes
    eng = engine.QcnnEngine(0, stream=stream.cuda_stream)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.load_model(in_chw, layers, synth.make_params(in_chw, layers, seed=0), SLOTS)
    prob = torch.empty((SLOTS, 1000), dtype=torch.float32, device="cuda")
    top5 = torch.empty((SLOTS, 5), dtype=torch.int16, device="cuda")
    calls = variants(eng, (prob.data_ptr(), top5.data_ptr(), None), ["bmp24"] if "bmp24" in letter else [])
    if "bmp24" in letter:
        calls[0][1]()
        eng.sync()
        p0, t0 = prob[:SLOTS // 10].clone(), top5[:SLOTS // 10].clone()
        calls[1][1]()
        eng.sync()
        same = bool(torch.equal(prob[:SLOTS // 10].view(torch.int32), p0.view(torch.int32)) and torch.equal(top5[:SLOTS // 10], t0))
        print("AlexNet from BMP files' bytes against from planar bytes (100 images x ten-crop): %s" % ("same bits" if same else "DIFFERENT"))
        if not same:
            sys.exit(1)
    report("whole call, AlexNet (prob + top-5 of the averaged rows), %d rounds:" % rounds, timed(stream, calls, rounds), yardstick_of)
    eng.close()

    # ---- the host work removed: de-interleave and flip the same files, one thread
    if "bmp24" in letter:
        print("host, one thread (OMP_NUM_THREADS=%s; numpy slicing and copy, no BLAS): BMP pixel array -> planar [3][h][w], top row first" % np_threads)
        for hs, ws in SIZES:
            files = strided[(hs, ws)]["bmp24"][0][:200].cpu().numpy()
            host_deinterleave(files[:20], hs, ws)
            per, out = host_deinterleave(files, hs, ws)
            if not np.array_equal(out, planar[(hs, ws)][0][:200].cpu().numpy()):
                print("the host's planar images differ from the device's")
                sys.exit(1)
            print("  %dx%d: %.3f ms an image, %.0f images/s, %.2f GB/s of planar bytes written" % (hs, ws, per * 1e3, 1.0 / per, 3 * hs * ws / per / 1e9))


if __name__ == "__main__":
    main()
