"""TEST INFRASTRUCTURE — the two streamed calls of tests/test_gpu_host_pipeline.py::test_debug_schedule_prints_one_ordered_line_per_batch:
float batches of 130, 1 and 257 images through forward_host_batches on the tiny model, then the smallest strict-mode 8-bit stream
tests/test_gpu_u8_stream.py builds (one view; batches of 1, 3 and 5 images).  The test calls run_calls() in its own process and
runs this file as a fresh child process with QCNN_DEBUG_PIPELINE=1 (the library reads the variable once per process):
    python pipeline_debug_calls.py OUT.npz      results into OUT.npz, MARK on stderr between the two calls."""
import os
import sys

import numpy as np

from conftest import GOLDEN, pkg, tiny_params_from_golden

FLOAT_SIZES = [130, 1, 257]
U8_COUNTS = (1, 3, 5)
MARK = "--- 8-bit stream ---"


def run_calls(between=lambda: None):
    """{name: array} of everything the two calls hand back; between() runs after the float call."""
    import test_gpu_u8_stream as us
    from u8_harness import make_engine
    topo, synth, capi, engine = pkg("topology"), pkg("synth"), pkg("capi"), pkg("engine")
    in_chw, layers = topo.tiny_model()
    out = {}
    eng = engine.QcnnEngine(0)
    eng.set_option(capi.OPT_LUT_MODE, capi.LUT_MFMA)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.set_option(capi.OPT_SMALL_BATCH, 0)
    eng.set_option(capi.OPT_SPLIT, 0)
    eng.load_model(in_chw, layers, synth.make_params(in_chw, layers, seed=21), max(FLOAT_SIZES))
    imgs = synth.make_images(sum(FLOAT_SIZES), in_chw, seed=22)
    offs = np.cumsum([0] + FLOAT_SIZES)
    prob, top5 = eng.forward_host_batches([imgs[offs[i]:offs[i + 1]] for i in range(len(FLOAT_SIZES))])
    eng.close()
    for b in range(len(FLOAT_SIZES)):
        out["float_prob_%d" % b], out["float_top5_%d" % b] = prob[b], top5[b]
    between()
    eng = make_engine(in_chw, layers, tiny_params_from_golden(np.load(os.path.join(GOLDEN, "tiny_ref.npz")), layers), 40, lut=capi.LUT_MFMA)
    bufs = us._buffers("tiny", U8_COUNTS, 860)
    outs = us.stream(eng, "strict", us.TINY_FULL, bufs, us.Mean(us._mean("tiny", "strict", 861)), us._views("tiny", "strict", 1))
    eng.close()
    for b, (p, t, r) in enumerate(outs):
        out["u8_prob_%d" % b], out["u8_top5_%d" % b], out["u8_rows_%d" % b] = p, t, r
    return out


if __name__ == "__main__":
    def mark():
        sys.stderr.flush()
        print(MARK, file=sys.stderr, flush=True)

    np.savez(sys.argv[1], **run_calls(mark))
