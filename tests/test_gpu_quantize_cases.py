"""qcnn_quantize_layer on the crafted cases of tests/pq_cases.py: exact ties for the nearest code word, tied farthest points in
one lane / one wave / two waves of the seed block, member sums that depend on the order, N around 64 / 128 / 256 / 4096 with
every N % 4, every (Cs, CsEff), code words without members, distances at both ends of the fp32 range, sub-spaces converging at
different steps.  Every case is held to the numpy oracle (tests/pq_oracle.py) bit for bit with the assertions of
test_gpu_quantize.check_vs_oracle; tests/test_pq_cases_cpu.py shows, without a GPU, that the oracle is the contract on these
cases and which wrong kernels each family would catch."""
import numpy as np
import pytest

import pq_cases as pc
import pq_oracle
from conftest import pkg

pytestmark = pytest.mark.gpu

engine = pkg("engine")


@pytest.fixture(scope="module")
def eng():
    e = engine.QcnnEngine(0)
    yield e
    e.close()


def check_case(eng, w, M, K, Cs, init, max_iter):
    """check_vs_oracle of test_gpu_quantize.py, restated with where the bytes differ in the message; then the padded dims as
    +0.0 bit for bit, and a second call with the same bytes and stats."""
    got = eng.quantize_layer(w, M, K, Cs, ctrd_init=init, max_iter=max_iter)
    with np.errstate(all="ignore"):
        want = pq_oracle.quantize_layer(w, M, K, Cs, ctrd_init=init, max_iter=max_iter)
    where = pc.describe_diff(got, want, M, K, Cs)
    assert got[0].tobytes() == want[0].tobytes(), "code book differs: " + where
    assert got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes(), "assignments differ: " + where
    gs, ws = got[2], want[2]
    assert (gs["iters"], gs["unconverged"]) == (ws["iters"], ws["unconverged"]), (gs, ws)
    for key in ("sse_init", "sse"):
        assert abs(gs[key] - ws[key]) <= 1e-9 * max(abs(ws[key]), 1e-30), (key, gs, ws)
    cse = np.asarray(w).shape[1] - (M - 1) * Cs
    assert got[0][M - 1, :, cse:].tobytes() == bytes(4 * K * (Cs - cse)), "padded dims are not +0.0"
    again = eng.quantize_layer(w, M, K, Cs, ctrd_init=init, max_iter=max_iter)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and again[2] == got[2], "second call differs"


@pytest.mark.parametrize("family", sorted(pc.FAMILIES))
def test_crafted_family_bit_identical_to_the_oracle(eng, family):
    failed = []
    cases = pc.FAMILIES[family]()
    for name, case in cases.items():
        try:
            check_case(eng, *case)
        except AssertionError as ex:
            failed.append("%s/%s: %s" % (family, name, str(ex).split("\n")[0]))
    assert not failed, "%d of %d cases:\n%s" % (len(failed), len(cases), "\n".join(failed))
