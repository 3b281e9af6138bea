"""TEST INFRASTRUCTURE — numpy restatement of the hit rule of qcnn_count_top5_hits / qcnn_forward_u8_*_host_batches (k_top5_hits of
quantized-cnn_amd/csrc/qcnn_glue.hip): the reference's CaffeEva::CalcPredAccu (src/CaffeEva.cc:276-286) BEFORE its running sum.

  hits[r] = #{ i : top5[i][r] == label[i] }        r = 0..4, one label per IMAGE, every rank tested by itself

A row that repeats a class counts it at every rank where it stands (the reference's rows repeat class 0 once fewer than five
probabilities exceed FLT_MIN).  The cumulative ACCURACY@k that Main.cc prints is the running sum over the ranks.  No GPU here:
tests/test_u8_stream_cpu.py holds this module to hand-made rows and to eight wrong copies of itself; tests/test_gpu_u8_stream.py
holds the kernel and the streamed calls to it exactly."""
import numpy as np


def hits5(top5, labels):
    """top5 [n][5], labels [n] -> uint64 [5]."""
    top5, labels = np.asarray(top5), np.asarray(labels)
    assert top5.ndim == 2 and top5.shape[1] == 5 and labels.shape == (top5.shape[0],)
    out = np.zeros(5, np.uint64)
    for i in range(top5.shape[0]):
        for r in range(5):
            if int(top5[i, r]) == int(labels[i]):
                out[r] += np.uint64(1)
    return out


def hits5_batches(top5s, labels, start=None):
    """The counters of a streamed call: the sum over its labelled batches (labels[b] None: batch not counted), on top of `start`."""
    out = np.zeros(5, np.uint64) if start is None else np.array(start, np.uint64)
    for t, l in zip(top5s, labels):
        if l is not None:
            out = out + hits5(t, l)
    return out


def accuracy(hits, n):
    """The five cumulative fractions: ACCURACY@k = (hits[0] + ... + hits[k-1]) / n."""
    run = np.cumsum(np.asarray(hits, np.uint64).astype(np.int64))
    return [float(int(v) / n) for v in run]
