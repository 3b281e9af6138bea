#!/usr/bin/env python3
"""Write tests/golden/resize_ref.npz: crafted 8-bit source planes and what the COMPILED REFERENCE's BmpImgIO::ReszImg makes of
them (oracle/_ref/libqcnn_ref.so through pyoracle.RefLib().load_bmp with a zero mean and crop = full: the bare resize result for
a square full image).  tests/test_resize_cpu.py holds tests/resize_ref.py to these bits.  Data only: the source planes, the full
sizes and the reference's outputs.  Needs the compiled reference; no GPU.
usage: make_resize_golden.py [out.npz]"""
import importlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import pyoracle as po       # noqa: E402
import resize_ref as rr     # noqa: E402

fileio = importlib.import_module("quantized-cnn_amd.fileio")

# (full, (h, w)): full - 1 = 11 and 13 are the destination sizes with rounding seams at these sources (tests/resize_ref.SOURCES);
# 30 only for general down- and upscales, so that the file stays small
CASES = [
    (12, (12, 12)), (12, (14, 14)), (12, (30, 30)), (12, (14, 30)), (12, (1, 1)), (12, (37, 53)),
    (14, (14, 14)), (14, (8, 8)), (14, (54, 54)), (14, (8, 54)), (14, (2, 2)), (14, (1, 9)), (14, (5, 100)),
    (30, (37, 53)), (30, (5, 7)),
]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "resize_ref.npz")
    ref = po.RefLib()
    rng = np.random.default_rng(20261019)
    arrays = {"full": np.array([c[0] for c in CASES], np.int32)}
    with tempfile.TemporaryDirectory() as d:
        for k, (full, (h, w)) in enumerate(CASES):
            src = rr.random_images(rng, 1, 3, [(h, w)])[0]
            mean, bmp = os.path.join(d, "mean%d.bin" % full), os.path.join(d, "case%d.bmp" % k)
            fileio.write_bin(mean, np.zeros((3, full, full), np.float32))
            rr.write_bmp(bmp, src)
            got = ref.load_bmp(mean, bmp, full, crop=full)[0]
            arrays["src_%02d" % k], arrays["out_%02d" % k] = src, got
            same = np.array_equal(got.view(np.uint32), rr.resize(src, full, full).view(np.uint32))
            print("case %2d: %3dx%-3d -> %dx%d  resize_ref %s" % (k, h, w, full, full, "same bits" if same else "DIFFERENT"))
    np.savez_compressed(out, **arrays)
    print("%s: %d bytes" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
