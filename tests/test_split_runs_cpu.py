"""The run order of k_conv_dec_nchw_split, modelled in numpy: every (channel, kernel row) of the window is cut into
ceil(knl / 4) runs of 4 consecutive columns, the last one moved back to end at the row's last column.  A lane reads a
run with ONE 16-byte load at the run's offset.  The decoder (k_decode_weights_split) gives k = 4 run + e the code word of
column start + e, zero where that column was covered by an earlier run of the row or past the last run.  These tests
restate both formulas and check that the kernel's reads and the decoder's code words describe the same sum."""
import itertools

import numpy as np
import pytest

LDS_LIMIT = 160 * 1024


def runs_per_row(cin, knl, ct):
    """nchw_split_runs: runs per kernel row of the run order, 0 = the flat order (its w1 / w2 + table do not fit LDS)."""
    if knl < 4:
        return 0
    nr = (knl + 3) // 4
    return nr if lds_bytes(kb_of(cin, knl, nr), ct, nr) <= LDS_LIMIT else 0


def kb_of(cin, knl, nr):
    return (cin * knl * nr + 7) // 8 * 32 if nr else (cin * knl * knl + 31) // 32 * 32


def lds_bytes(kb, ct, nr):
    return kb * ct * 4 + (kb // 4 + 8 if nr else kb + 32) * 4


def run_table(cin, knl, nr, kb, H, W):
    """The kernel's LDS table: byte offset of run i inside an image, runs past the last repeat it (kb / 4 + 8 entries)."""
    n_runs = cin * knl * nr
    out = []
    for i in range(kb // 4 + 8):
        r = min(i, n_runs - 1)
        kw, kh, c = min(4 * (r % nr), knl - 4), (r // nr) % knl, r // (nr * knl)
        out.append(c * H * W * 4 + kh * W * 4 + kw * 4)
    return np.array(out, np.int64)


def decoder(cin, knl, nr, kb):
    """k_decode_weights_split's window element per k: (c, kh, kw) or None where the code word is zero."""
    out = []
    for k in range(kb):
        r, ri = k >> 2, (k >> 2) % nr
        kw, kh, c = min(4 * ri, knl - 4) + (k & 3), (r // nr) % knl, r // (nr * knl)
        live = r < cin * knl * nr and kw >= 4 * ri
        out.append((c, kh, kw) if live else None)
    return out


SHAPES = [(cin, knl, stride) for cin, knl, stride in itertools.product(range(1, 5), range(3, 13), range(1, 6))]


@pytest.mark.parametrize("cin,knl,stride", SHAPES)
def test_run_table(cin, knl, stride):
    ct = 96
    nr = runs_per_row(cin, knl, ct)
    if knl < 4:
        assert nr == 0                                    # rows shorter than a run: the flat order
        return
    if not nr:                                            # too large for LDS in run order: the flat order or no split
        nr = (knl + 3) // 4                               # path at all (the run order's table is still checked below)
        assert lds_bytes(kb_of(cin, knl, nr), ct, nr) > LDS_LIMIT
    kb = kb_of(cin, knl, nr)
    assert kb % 32 == 0 and kb >= cin * knl * nr * 4
    Wo = 3
    H, W = knl + 2, (Wo - 1) * stride + knl               # the last output column's window ends at the row's end
    tab = run_table(cin, knl, nr, kb, H, W)
    dec = decoder(cin, knl, nr, kb)
    seen = {}
    for k in range(kb):
        # what the kernel reads for k: element k & 3 of the 16-byte load at the run's offset (the image, output position
        # and row of the tile are in the scalar / lane offsets, as before)
        addr = tab[k >> 2] + 4 * (k & 3)
        c, rem = divmod(int(addr), H * W * 4)
        kh, col4 = divmod(rem, W * 4)
        kw = col4 // 4
        assert c < cin and kh < knl and kw < knl, (k, c, kh, kw)      # the read stays inside the window's row
        for pos in range(Wo):                                         # ... and inside the image row at every position
            assert pos * stride + kw < W
        if dec[k] is not None:
            assert dec[k] == (c, kh, kw), (k, dec[k], (c, kh, kw))    # the code word belongs to the element read
            assert dec[k] not in seen, (k, dec[k])
            seen[dec[k]] = k
    window = {(c, kh, kw) for c in range(cin) for kh in range(knl) for kw in range(knl)}
    assert set(seen) == window                            # every window element exactly once with its code word
    # the repeated columns: exactly the row's last-run overlap, zero code words
    zeros_in_runs = sum(1 for k in range(cin * knl * nr * 4) if dec[k] is None)
    assert zeros_in_runs == cin * knl * (4 * nr - knl)
    # every run offset starts a 16-byte read that ends inside its window row
    for i in range(kb // 4 + 8):
        rem = int(tab[i]) % (W * 4)
        assert rem // 4 + 3 <= knl - 1


def test_alexnet_budget():
    """AlexNet's conv1 (3 x 11 x 11, 96 channels) takes the run order: 396 k in 13 steps of 32, w1 / w2 and the table
    inside LDS; (Cin 4, knl 9) keeps the flat order."""
    assert runs_per_row(3, 11, 96) == 3 and kb_of(3, 11, 3) == 416
    assert lds_bytes(416, 96, 3) == 416 * 96 * 4 + 112 * 4 <= LDS_LIMIT
    assert runs_per_row(4, 9, 96) == 0 and kb_of(4, 9, 0) == 352
    assert runs_per_row(1, 3, 96) == 0
