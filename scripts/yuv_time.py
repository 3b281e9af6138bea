#!/usr/bin/env python3
"""What reading YCbCr frames in place costs and saves (LABBOOK.md, "YCbCr sources"): qcnn_forward_u8_resized_views_yuv against
qcnn_forward_u8_resized_views_strided on interleaved B, G, R bytes of the SAME images (the integer conversion of the frames,
done here on the device), full image 256 x 256 with a mean image, sources of 256 x 256 and of 500 x 375.

  pack     the rig of scripts/layout_time.py: 1000 batch slots as 100 images x ten-crop and as 1000 images x the centre view.
             (c) bgr    interleaved [h][w][3], tight: layout_time's row (c), an existing kernel
             NV12       luma plane, then interleaved Cb Cr rows of half the height
             I420       three planes, chroma 2 x 2 sub-sampled
             I444       three planes of full size (chroma replicated, so that the picture is the same)
           pack step: a glue-only model ([relu]) of AlexNet's input shape, no output asked for, HIP events around a call.
           Bar: an NV12 pack step takes at most 13 / 5 = 2.6 x the bgr pack step of the same shape, the ratio of loads issued
           per slot-element (twelve tap bytes and the mean against four and the mean).
           whole call: AlexNet with synthetic parameters, prob + top-5, from NV12 against from bgr (reported, no bar).
  stream   the rig of scripts/stream_time.py: 500 x 375 sources, 1000 images x the centre view, BATCHES batches from
           qcnn_host_alloc memory; qcnn_forward_u8_resized_host_batches_yuv on NV12 frames (282 MB a batch) against
           qcnn_forward_u8_resized_host_batches on the bgr bytes (562.5 MB), alternating, host clock around the blocking call.

Before anything is timed the frames and their bgr conversion must give the same bits (fm[0] of the first slots; batch 0).
usage: yuv_time.py pack [rounds=20] [--pack-only]
       yuv_time.py stream [batches=8] [reps=5] [--schedule]     --schedule: QCNN_DEBUG_PIPELINE=1 and one call of each"""
import importlib, os, sys, time
if "--schedule" in sys.argv:
    os.environ["QCNN_DEBUG_PIPELINE"] = "1"           # read once, when the library first streams
import numpy as np
import torch   # before libqcnn_hip.so: both must bind to the HIP runtime torch ships
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n: importlib.import_module("quantized-cnn_amd." + n)

FULL = (256, 256)
SLOTS = 1000
SIZES = ((256, 256), (500, 375))
JFIF = (0, 65536, 91881, 22554, 46802, 116130)


def frames_on_device(engine, n, h, w, seed):
    """n random frames -> {name: (device buffer, descriptors)} for NV12, I420, I444 and the bgr bytes of their conversion."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    Y = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda", generator=g)
    Cb, Cr = (torch.randint(0, 256, (n, ch, cw), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2))
    pitch = 2 * cw
    nv12 = torch.zeros((n, h + ch, pitch), dtype=torch.uint8, device="cuda")
    nv12[:, :h, :w] = Y
    nv12[:, h:, 0::2] = Cb
    nv12[:, h:, 1::2] = Cr
    i420 = torch.cat([Y.reshape(n, -1), Cb.reshape(n, -1), Cr.reshape(n, -1)], dim=1).contiguous()
    rep = lambda p: p.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :h, :w]
    i444 = torch.stack([Y, rep(Cb), rep(Cr)], dim=1).contiguous()
    bgr = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    y0, ky, crv, cbg, crg, cbu = JFIF
    for a in range(0, n, 50):                          # the table of include/qcnn_hip.h in int32
        yy = (Y[a:a + 50].to(torch.int32) - y0) * ky
        cb, cr = rep(Cb[a:a + 50]).to(torch.int32) - 128, rep(Cr[a:a + 50]).to(torch.int32) - 128
        for c, v in enumerate((yy + cbu * cb, yy - cbg * cb - crg * cr, yy + crv * cr)):
            bgr[a:a + 50, :, :, c] = ((v + 32768) >> 16).clamp_(0, 255).to(torch.uint8)
    sizes = {"NV12": nv12[0].numel(), "I420": i420[0].numel(), "I444": i444[0].numel()}
    out = {"bgr": (bgr, engine._pixels_array([engine.SrcPixels(i * 3 * h * w, 3 * w, h, w, 3, (0, 1, 2, 0)) for i in range(n)])[0])}
    for name, buf in (("NV12", nv12), ("I420", i420), ("I444", i444)):
        out[name] = (buf, engine._yuv_array([engine.src_yuv_frame(name, i * sizes[name], h, w) for i in range(n)])[0])
    return out


def call_of(eng, name):
    return eng.forward_u8_resized_views_strided_dev if name == "bgr" else eng.forward_u8_resized_views_yuv_dev


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


def report(title, ms, bar=None):
    print(title)
    over = []
    for name, v in ms.items():
        base = float(np.median(ms["bgr   " + name[6:]]))
        ratio = float(np.median(v)) / base
        print("  %-40s median %.3f ms  (min %.3f - max %.3f)  x %.3f of bgr" % (name, float(np.median(v)), min(v), max(v), ratio))
        if bar and name.startswith("NV12") and ratio > bar:
            over.append((name, ratio))
    if bar:
        print("  bar: NV12 at most %.1f x bgr: %s" % (bar, "MISSED by %r" % over if over else "held in every shape"))


def pack(rounds, pack_only):
    capi, topo, synth, engine = pkg("capi"), pkg("topology"), pkg("synth"), pkg("engine")
    in_chw, layers, _, _ = topo.MODELS["AlexNet"]
    c, h, w = in_chw
    rng = np.random.default_rng(9)
    mean = torch.from_numpy((rng.standard_normal((c,) + FULL) * 20 + 110).astype(np.float32)).cuda()
    ten = engine.ten_crop_views(FULL[0], FULL[1], h, w)
    frames = {size: frames_on_device(engine, SLOTS, size[0], size[1], 11 + k) for k, size in enumerate(SIZES)}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    shapes = ((SLOTS // 10, ten, "%d x ten-crop" % (SLOTS // 10)), (SLOTS, [ten[4]], "%d x centre" % SLOTS))

    def variants(eng, outs, names):
        calls = []
        for n, views, label in shapes:
            for size in SIZES:
                for name in names:
                    buf, descs = frames[size][name]
                    sub = type(descs)._type_ * n
                    d = sub.from_buffer(descs)          # the first n descriptors
                    calls.append(("%-5s %dx%d  %s" % (name, size[0], size[1], label), lambda n=n, views=views, buf=buf, d=d, name=name: call_of(eng, name)(
                        buf.data_ptr(), buf.numel(), d, FULL[0], FULL[1], mean.data_ptr(), views, *outs)))
        return calls

    glue = engine.QcnnEngine(0, stream=stream.cuda_stream)
    glue.set_option(capi.OPT_KEEP_ALL, 1)
    glue.load_model(in_chw, [topo.relu()], {}, SLOTS)
    calls = variants(glue, (None, None, None), ["bgr", "NV12", "I420", "I444"])
    want = {}
    for name, call in calls:                            # the same picture under every layout: the same bits
        call()
        glue.sync()
        got = glue.layer_output_range(0, 0, 16).view(np.uint32)
        if not np.array_equal(want.setdefault(name[6:], got), got):
            print("fm[0] under %s differs from the bgr call's" % name)
            sys.exit(1)
    print("fm[0] of the first 16 slots: the same bits from bgr, NV12, I420 and I444, every source size and slot shape")
    report("pack kernel + one ReLU sweep over %d x %d floats (glue-only model), %d rounds:" % (SLOTS, c * h * w, rounds),
           timed(stream, calls, rounds), bar=2.6)
    glue.close()
    if pack_only:
        return
    eng = engine.QcnnEngine(0, stream=stream.cuda_stream)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.load_model(in_chw, layers, synth.make_params(in_chw, layers, seed=0), SLOTS)
    prob = torch.empty((SLOTS, 1000), dtype=torch.float32, device="cuda")
    top5 = torch.empty((SLOTS, 5), dtype=torch.int16, device="cuda")
    calls = variants(eng, (prob.data_ptr(), top5.data_ptr(), None), ["bgr", "NV12"])
    calls[0][1]()
    eng.sync()
    p0, t0 = prob[:SLOTS // 10].clone(), top5[:SLOTS // 10].clone()
    calls[1][1]()
    eng.sync()
    same = bool(torch.equal(prob[:SLOTS // 10].view(torch.int32), p0.view(torch.int32)) and torch.equal(top5[:SLOTS // 10], t0))
    print("AlexNet from NV12 frames against from their bgr bytes (100 images x ten-crop): %s" % ("same bits" if same else "DIFFERENT"))
    if not same:
        sys.exit(1)
    report("whole call, AlexNet (prob + top-5 of the averaged rows), %d rounds:" % rounds, timed(stream, calls, rounds))
    eng.close()


def stream(nb, reps, schedule):
    capi, topo, synth, engine = pkg("capi"), pkg("topology"), pkg("synth"), pkg("engine")
    in_chw, layers, _, _ = topo.MODELS["AlexNet"]
    c, h, w = in_chw
    hs, ws = SIZES[1]
    rng = np.random.default_rng(9)
    d_mean = torch.from_numpy((rng.standard_normal((c,) + FULL) * 20 + 110).astype(np.float32)).cuda()
    views = [engine.ten_crop_views(FULL[0], FULL[1], h, w)[4]]
    st = torch.cuda.Stream()
    eng = engine.QcnnEngine(0, stream=st.cuda_stream)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.load_model(in_chw, layers, synth.make_params(in_chw, layers, seed=0), SLOTS)
    dev = frames_on_device(engine, SLOTS, hs, ws, 12)
    host, batches, outs = {}, {}, {}
    for name in ("bgr", "NV12"):
        flat = dev[name][0].reshape(-1).cpu().numpy()
        host[name] = [engine.host_alloc(flat.size) for _ in range(2)]     # two pinned buffers, the batches alternating between them
        for p in host[name]:
            p[:] = flat
        batches[name] = [(host[name][b & 1], dev[name][1]) for b in range(nb)]
        outs[name] = [(np.empty((SLOTS, 1000), np.float32), np.empty((SLOTS, 5), np.uint16), None) for _ in range(nb)]
    del dev
    torch.cuda.synchronize()
    call = {name: (lambda name=name: eng.forward_u8_host_batches_into(batches[name], FULL, d_mean.data_ptr(), views, "strict", outs[name]))
            for name in ("bgr", "NV12")}
    print("AlexNet, %dx%d sources, %d x centre, %d batches a call from pinned memory: bgr %.1f MB a batch, NV12 %.1f MB" %
          (hs, ws, SLOTS, nb, host["bgr"][0].size / 1e6, host["NV12"][0].size / 1e6))
    for name in ("bgr", "NV12"):
        if schedule:
            print("schedule of the %s stream:" % name, file=sys.stderr)
        call[name]()
    same = np.array_equal(outs["bgr"][0][0].view(np.uint32), outs["NV12"][0][0].view(np.uint32)) and np.array_equal(outs["bgr"][0][1], outs["NV12"][0][1])
    print("  batch 0 of the NV12 stream against the bgr stream: %s" % ("same bits" if same else "DIFFERENT"))
    if not same:
        sys.exit(1)
    if not schedule:
        ms = {name: [] for name in call}
        for _ in range(reps):
            for name in ("bgr", "NV12"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call[name]()
                ms[name].append((time.perf_counter() - t0) * 1e3 / nb)
        for name, v in ms.items():
            print("  %-5s stream  ms PER BATCH: median %.3f (min %.3f - max %.3f), %d repetitions" % (name, float(np.median(v)), min(v), max(v), reps))
        print("  NV12 / bgr = %.3f; NV12 maximum %.3f ms against bgr minimum %.3f ms: %s" % (
            float(np.median(ms["NV12"])) / float(np.median(ms["bgr"])), max(ms["NV12"]), min(ms["bgr"]),
            "below" if max(ms["NV12"]) < min(ms["bgr"]) else "NOT below"))
    for ps in host.values():
        for p in ps:
            engine.host_free(p)
    eng.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if not args or args[0] not in ("pack", "stream"):
        sys.exit(__doc__)
    nums = [int(a) for a in args[1:]]
    if args[0] == "pack":
        pack(nums[0] if nums else 20, "--pack-only" in sys.argv)
    else:
        stream(nums[0] if nums else 8, nums[1] if len(nums) > 1 else 5, "--schedule" in sys.argv)
