"""TEST HELPER — crafted layers for qcnn_quantize_layer and a scalar restatement of its contract (DESIGN.md "Quantising dense
weights"), one point, one code word and one coordinate at a time.

``quantize_layer`` here has the signature and outputs of ``pq_oracle.quantize_layer`` and shares no code with it: numpy.float32
scalars for ``t = p - c; d = d + t * t``, ``if d < best`` for the assign rule, ``if d > best`` for the seed rule, a Python float
running sum in ascending n and ``np.float32(s / cnt)`` for the update.  It is slow by design and meant for the crafted cases
below only.  ``wrong`` switches single mistakes on (WRONG); ``trace`` (a dict) receives what the potency conditions of
tests/test_pq_cases_cpu.py are asserted on.

Every family is a function returning ``{name: (weights, M, K, Cs, ctrd_init or None, max_iter)}``; FAMILIES names them.  The
inputs on which the rules of the contract decide bytes: exact ties for the nearest code word, tied farthest points at chosen
places of the 256-lane seed block, member sums whose fp64 value depends on the order, N around the wave / block / staging-chunk
sizes, every (Cs, CsEff), code words without members, distances at both ends of the fp32 range, sub-spaces that converge at
different steps.
"""
from __future__ import annotations

import numpy as np

F = np.float32
FLT_MIN = 2.0 ** -126                  # smallest normal float32
FLT_MAX = float(np.finfo(np.float32).max)
SEED_BLOCK, WAVE = 256, 64             # k_pq_seed: lane = n % 256, wave = lane // 64
CHUNK = 4096                           # k_pq_update stages this many assignment bytes at a time, four to a read

WRONG = ("assign_le",                  # '<=' in assign: ties go to the highest k
         "seed_highest",               # seed ties go to the highest n
         "seed_lane_last",             # the last maximum within a lane of the seed block (n, n + 256, ...) stays
         "seed_wave_highest",          # ties between two lanes of a wave go to the higher n
         "seed_block_highest",         # ties between two waves go to the higher n
         "sum_reversed",               # member sum in descending n
         "sum_pairwise",               # member sum as a balanced tree
         "sum_interleave4",            # four running sums over the points n % 4, added at the end
         "sum_fp32",                   # member sum in float32
         "div_float",                  # (float)S / (float)count
         "empty_zero",                 # a code word without members becomes 0
         "pad_keep",                   # the padded dims of a given book are returned as given
         "dist_ftz",                   # subnormal results of the distance sequence flushed to zero
         "tail_dropped")               # members at n >= 4 * (len // 4) of a staging chunk left out


# ------------------------------------------------------------------------------ the scalar reference
def _dist(p, c, cse):
    d = F(0.0)
    for j in range(cse):
        t = p[j] - c[j]
        d = d + t * t
    return d


def _flush(x):
    return F(0.0) if abs(x) < FLT_MIN else x


def _dist_ftz(p, c, cse):
    d = F(0.0)
    for j in range(cse):
        t = _flush(_flush(p[j]) - _flush(c[j]))
        d = _flush(d + _flush(t * t))
    return d


def _assign(pts, book, cse, dist, le):
    """(assignments, minimum distances, points with an exact tie for the minimum, largest distance seen)."""
    a, dm, tied, dmax = [], [], 0, F(0.0)
    for p in pts:
        best, bk, nmin = dist(p, book[0], cse), 0, 1
        if best > dmax:
            dmax = best
        for k in range(1, len(book)):
            d = dist(p, book[k], cse)
            if d > dmax:
                dmax = d
            if d < best:
                best, bk, nmin = d, k, 1
            elif d == best:
                nmin += 1
                if le:
                    bk = k
        a.append(bk)
        dm.append(best)
        tied += nmin > 1
    return a, dm, tied, dmax


def argmax_block(d, lane_last=False, wave_highest=False, block_highest=False):
    """The argmax as a 256-lane block finds it: every lane scans n = lane, lane + 256, ..., the lanes of a wave are compared,
    then the waves.  With no switch set this is the first maximum (ties to the lowest n); each switch turns one level's tie
    rule round."""
    lanes = []
    for lane in range(SEED_BLOCK):
        best, bn = F(-1.0), 0
        for n in range(lane, len(d), SEED_BLOCK):
            if d[n] > best or (lane_last and d[n] == best):
                best, bn = d[n], n
        lanes.append((best, bn))

    def fold(items, highest):
        best, bn = items[0]
        for ob, on in items[1:]:
            if ob > best or (ob == best and (on > bn if highest else on < bn)):
                best, bn = ob, on
        return best, bn

    waves = [fold(lanes[w:w + WAVE], wave_highest) for w in range(0, SEED_BLOCK, WAVE)]
    return fold(waves, block_highest)[1]


def _seed(pts, K, cse, dist, wrong, rounds):
    """Farthest-first: c_0 = point 0, then the point farthest from its nearest chosen code word, the first such n.  rounds
    receives (the n at which the maximum is attained, the n picked) of every round."""
    N = len(pts)
    dmin = [None] * N
    cur, book, dmax = 0, [list(pts[0])], F(0.0)
    for i in range(1, K):
        c = pts[cur]
        best, bn = F(-1.0), 0
        for n in range(N):
            d = dist(pts[n], c, cse)
            if d > dmax:
                dmax = d
            if i > 1 and dmin[n] < d:
                d = dmin[n]
            dmin[n] = d
            if d > best or (d == best and "seed_highest" in wrong):
                best, bn = d, n
        hier = dict(lane_last="seed_lane_last" in wrong, wave_highest="seed_wave_highest" in wrong,
                    block_highest="seed_block_highest" in wrong)
        if any(hier.values()):
            bn = argmax_block(dmin, **hier)
        rounds.append(([n for n in range(N) if dmin[n] == best], bn))
        cur = bn
        book.append(list(pts[cur]))
    return book, dmax


def _tree(v):
    if len(v) == 1:
        return v[0]
    h = len(v) // 2
    return _tree(v[:h]) + _tree(v[h:])


def _update(pts, book, a, cse, wrong, sums):
    """Per code word with members float32(S / count), S the fp64 sum of the members' coordinates in ascending n; a code word
    without members keeps its value."""
    N = len(pts)
    members = [[] for _ in book]
    for n in range(N):
        if "tail_dropped" in wrong:
            n0 = n - n % CHUNK
            if n - n0 >= (min(CHUNK, N - n0) // 4) * 4:
                continue
        members[a[n]].append(n)
    new = []
    for k, mem in enumerate(members):
        if not mem:
            new.append([F(0.0)] * cse if "empty_zero" in wrong else list(book[k]))
            continue
        cnt = len(mem)
        word = []
        for j in range(cse):
            if "sum_fp32" in wrong:
                s = F(0.0)
                for n in mem:
                    s = s + pts[n][j]
                s = float(s)
            elif "sum_pairwise" in wrong:
                s = _tree([float(pts[n][j]) for n in mem])
            elif "sum_interleave4" in wrong:
                acc = [0.0, 0.0, 0.0, 0.0]
                for n in mem:
                    acc[n % 4] += float(pts[n][j])
                s = (acc[0] + acc[1]) + (acc[2] + acc[3])
            else:
                s = 0.0
                for n in (reversed(mem) if "sum_reversed" in wrong else mem):
                    s += float(pts[n][j])
            if sums is not None:
                sums.append((k, j, [float(pts[n][j]) for n in mem], s))
            word.append(F(F(s) / F(cnt)) if "div_float" in wrong else F(s / cnt))
        new.append(word)
    return new, members


def quantize_layer(w, M, K, Cs, ctrd_init=None, max_iter=30, wrong=(), trace=None):
    """(ctrd [M][K][Cs], asmt in file order, stats dict(sse_init, sse, iters, unconverged)) of the contract, by plain loops.
    trace, per sub-space m: ties[m] the tied points of every assign, rounds[m] the seed rounds, steps[m], changing[m],
    dmax[m] the largest distance computed, dm[m] the final minimum distances, sums[m] [(step, k, j, member values, S)],
    never_member[m] the code words that had no member at any update."""
    wrong = tuple(wrong)
    assert all(x in WRONG for x in wrong), wrong
    w = np.asarray(w, np.float32)
    if w.ndim == 4:
        ct, cin, kh, kw = w.shape
        ashape = (ct, kh, kw, M)
    else:
        (ct, cin), kh, kw = w.shape, 1, 1
        ashape = (ct, M)
    taps = kh * kw
    N = ct * taps
    w3 = w.reshape(ct, cin, taps)
    dist = _dist_ftz if "dist_ftz" in wrong else _dist
    C = np.zeros((M, K, Cs), np.float32)
    if ctrd_init is not None:
        init = np.asarray(ctrd_init, np.float32)
        if "pad_keep" in wrong:
            C[:] = init
    A = np.zeros((N, M), np.uint8)
    sse0 = sse1 = 0.0
    iters = unconverged = 0
    with np.errstate(all="ignore"):
        for m in range(M):
            cse = min(cin - m * Cs, Cs)
            pts = [[w3[n // taps, m * Cs + j, n % taps] for j in range(cse)] for n in range(N)]
            rounds, ties, sums = [], [], []
            if ctrd_init is not None:
                book, dmax = [[init[m, k, j] for j in range(cse)] for k in range(K)], F(0.0)
            else:
                book, dmax = _seed(pts, K, cse, dist, wrong, rounds)
            a, dm, tied, dx = _assign(pts, book, cse, dist, "assign_le" in wrong)
            ties.append(tied)
            dmax = max(dmax, dx)
            for d in dm:
                sse0 += float(d)
            steps, changing = 0, False
            never = set(range(K))
            for _ in range(max_iter):
                step_sums = [] if trace is not None else None
                book, members = _update(pts, book, a, cse, wrong, step_sums)
                never -= {k for k in range(K) if members[k]}
                if step_sums:
                    sums += [(steps,) + s for s in step_sums]
                a2, dm, tied, dx = _assign(pts, book, cse, dist, "assign_le" in wrong)
                ties.append(tied)
                dmax = max(dmax, dx)
                steps += 1
                changing = a2 != a
                a = a2
                if not changing:
                    break
            iters = max(iters, steps)
            unconverged += bool(changing)
            for d in dm:
                sse1 += float(d)
            for k in range(K):
                for j in range(cse):
                    C[m, k, j] = book[k][j]
            A[:, m] = a
            if trace is not None:
                for key, val in (("ties", ties), ("rounds", rounds), ("steps", steps), ("changing", bool(changing)),
                                 ("dmax", float(dmax)), ("dm", [float(d) for d in dm]), ("sums", sums),
                                 ("never_member", sorted(never) if max_iter else []), ("pts", pts)):
                    trace.setdefault(key, {})[m] = val
    return C, A.reshape(ashape), dict(sse_init=sse0, sse=sse1, iters=iters, unconverged=unconverged)


def describe_diff(got, want, M, K, Cs):
    """Where two (ctrd, asmt, stats) results first differ: sub-space, code word, dim / point — for failure messages."""
    out = []
    gc, wc = np.asarray(got[0]).view(np.uint32).reshape(M, K, Cs), np.asarray(want[0]).view(np.uint32).reshape(M, K, Cs)
    bad = np.argwhere(gc != wc)
    if len(bad):
        m, k, j = (int(v) for v in bad[0])
        out.append("book: %d entries differ, first [m=%d][k=%d][j=%d] got %r (0x%08x) want %r (0x%08x)"
                   % (len(bad), m, k, j, float(got[0][m, k, j]), gc[m, k, j], float(want[0][m, k, j]), wc[m, k, j]))
    ga, wa = np.asarray(got[1]).reshape(-1, M), np.asarray(want[1]).reshape(-1, M)
    if ga.shape != wa.shape:
        out.append("assignment shapes %r / %r" % (np.asarray(got[1]).shape, np.asarray(want[1]).shape))
    else:
        bad = np.argwhere(ga != wa)
        if len(bad):
            n, m = (int(v) for v in bad[0])
            out.append("assignments: %d differ, first [n=%d][m=%d] got %d want %d" % (len(bad), n, m, ga[n, m], wa[n, m]))
    if got[2] != want[2]:
        out.append("stats got %r want %r" % (got[2], want[2]))
    return "; ".join(out)


# ------------------------------------------------------------------------------ helpers of the case families
def _fc(subs):
    """Sub-space point sets [N][CsEff(m)] side by side: the FC layer [N][Cin] that holds them."""
    return np.ascontiguousarray(np.concatenate([np.asarray(s, np.float32) for s in subs], axis=1))


def _book(words, Cs, pad=0.0):
    """words [M][K][CsEff(m)] -> [M][K][Cs], the padded dims holding pad."""
    out = np.full((len(words), len(words[0]), Cs), pad, np.float32)
    for m, wm in enumerate(words):
        wm = np.asarray(wm, np.float32)
        out[m, :, :wm.shape[1]] = wm
    return out


def _bits(*patterns):
    return np.array(patterns, np.uint32).view(np.float32)


# ------------------------------------------------------------------------------ ties_assign
def ties_assign():
    """Integer points and books with duplicated and symmetrically placed code words: every sum of squares is exact, and many
    points have several nearest code words at exactly the same distance.  Only '<' sends them to the lowest k."""
    cases = {}
    rng = np.random.default_rng(101)
    grid = np.array([(x, y) for x in range(-3, 4) for y in range(-3, 4)], np.float32)            # 49 points
    subs = [grid[rng.permutation(49)], grid[rng.permutation(49)][:, ::-1], (np.arange(49).reshape(49, 1) * 5) % 7 - 3.0]
    book = _book([[(0, 0), (2, 0), (2, 0), (0, 2), (-2, 0), (0, 0)],
                  [(1, 1), (-1, -1), (1, -1), (-1, 1), (1, 1), (3, 3)],
                  [(0,), (2,), (2,), (-2,), (0,), (4,)]], 2)
    for it in (0, 3):
        cases["grid_m3_partial_iter%d" % it] = (_fc(subs), 3, 6, 2, book, it)                      # Cin = 5: CsEff = 1 last
    pts = rng.integers(-4, 5, (300, 5)).astype(np.float32)                                       # Cs = 3, CsEff = 2 last
    words = [np.concatenate([pts[:128, 0:3]] * 2), np.concatenate([pts[:128, 3:5]] * 2)]         # word k + 128 = word k
    for it in (0, 2):
        cases["dup_k256_iter%d" % it] = (pts, 2, 256, 3, _book(words, 3), it)
    conv = rng.integers(-1, 2, (6, 4, 2, 2)).astype(np.float32)                                   # conv layer: N = 24, Cs = 4
    sym = _book([[(1, 1, 1, 1), (-1, -1, -1, -1), (1, -1, 1, -1), (-1, 1, -1, 1)]], 4)
    for it in (0, 2):
        cases["conv_sym_iter%d" % it] = (conv, 1, 4, 4, sym, it)
    return cases


# ------------------------------------------------------------------------------ ties_seed
def _pair_subspace(N, pairs, radii, s):
    """[N][8]: the origin everywhere but at the pairs (na, nb), which hold r e_d + s e_d' and r e_d - s e_d' — two
    different points at the same distance from the origin and 4 s^2 from each other.  With decreasing radii, round i of the
    seeding sees exactly the two points of pair i at the maximum; afterwards the unpicked partners all sit at 4 s^2."""
    p = np.zeros((N, 8), np.float32)
    for i, ((na, nb), r) in enumerate(zip(pairs, radii)):
        d, sign = 2 * (i % 4), (1.0 if i < 4 else -1.0)
        p[na, d], p[na, d + 1] = sign * r, s
        p[nb, d], p[nb, d + 1] = sign * r, -s
    return p


def ties_seed():
    """No given book.  In every round the farthest-point maximum is attained at several n; in 'pairs' the two candidates of
    a round are different points placed in one lane of the 256-lane seed block (n, n + 256), in two lanes of one wave, or
    in two waves, so each level of the block argmax decides a round on its own."""
    cases = {}
    lane = [(7, 263), (300, 556), (20, 276)]
    wave = [(70, 100), (150, 386), (5, 6)]
    block = [(10, 200), (66, 400)]
    order0 = [lane[0], wave[0], block[0], lane[1], wave[1], block[1], lane[2], wave[2]]
    order1 = [block[1], wave[2], lane[2], block[0], lane[0], wave[1], wave[0], lane[1]]
    radii = [40.0 - 4.0 * i for i in range(8)]
    subs = [_pair_subspace(600, order0, radii, 1.0), _pair_subspace(600, order1, [r + 1.0 for r in radii], 2.0)]
    cases["pairs_m2"] = (_fc(subs), 2, 16, 8, None, 2)
    cases["pairs_first8"] = (_fc(subs[:1]), 1, 9, 8, None, 0)                  # only the eight two-candidate rounds
    cases["identical"] = (np.tile(np.array([[3.0, -2.0]], np.float32), (300, 1)), 1, 5, 2, None, 2)
    cases["n5_k8"] = (np.array([[0], [3], [-3], [-3], [3]], np.float32), 1, 8, 1, None, 2)     # N < K
    rng = np.random.default_rng(102)
    small = rng.integers(-2, 3, (20, 2)).astype(np.float32)
    small[0] = 0
    cases["n40_k256"] = (np.tile(small, (2, 1)), 1, 256, 2, None, 1)            # N < K, every point is there twice
    lat = rng.integers(-2, 3, (700, 3)).astype(np.float32)                      # Cs = 2, CsEff = 1 last
    lat[0] = 0
    cases["lattice_m2"] = (lat, 2, 5, 2, None, 3)
    return cases


# ------------------------------------------------------------------------------ sum_order
BIG = 2.0 ** 55                        # ulp 8 in fp64: a value below 4 added to it is lost
SUM_ORDER_EXACT = ("gauss_n4103",)     # Gaussian members add exactly in fp64: there for the division and the fp32 sum


def _sum_order_case(N, bigs, seed, far_every=97):
    """One dim, book (0, 2^58, -2^58): the values below 4 and +-2^55 all belong to code word 0, whose fp64 sum in ascending n
    loses every small value met between a +2^55 and the -2^55 after it; every far_every-th point belongs to code word 1."""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 16, N) * 0.25
    for n in range(far_every // 2, N, far_every):
        x[n] = 2.0 ** 58 * (1.0 + (n % 3) / 8.0)
    for n, v in bigs:
        x[n] = v
    book = _book([[(0.0,), (2.0 ** 58,), (-2.0 ** 58,)]], 1)
    return (x.astype(np.float32).reshape(N, 1), 1, 3, 1, book, 1)


def sum_order():
    """A given book and one step, so the members are known.  +-2^55 among values below 4 make a code word's fp64 sum depend
    on the order; the pairs straddle a four-assignment word, the tail of a chunk (N % 4 != 0) and the 4096 seam."""
    cases = {}
    cases["n11_word_and_tail"] = _sum_order_case(11, [(2, BIG), (5, -BIG), (6, BIG), (9, -BIG)], 201, far_every=7)
    cases["n4103_seam_and_tail"] = _sum_order_case(
        4103, [(100, BIG), (3001, -BIG), (4094, BIG), (4097, -BIG), (4099, BIG), (4101, -BIG)], 202)
    cases["n8195_two_seams"] = _sum_order_case(
        8195, [(5, BIG), (6, -BIG), (4090, BIG), (4098, -BIG), (8190, BIG), (8193, -BIG)], 203)
    rng = np.random.default_rng(204)
    w = rng.standard_normal((4103, 5)).astype(np.float32)                       # Cs = 3, CsEff = 2 last
    cases["gauss_n4103"] = (w, 2, 5, 3, _book([w[10:15, 0:3], w[20:25, 3:5]], 3), 1)
    return cases


# ------------------------------------------------------------------------------ sizes
SIZES = (1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 4099, 8195)


def sizes():
    """FC layers with Ct = N around the wave (64), the assign block (128), the seed block (256) and the staging chunk
    (4096), N % 4 of every kind, N < K included.  K = 256 runs with a given book at every N, seeded at every N up to 257 and
    at 4097."""
    cases = {}
    for N in SIZES:
        rng = np.random.default_rng(300 + N)
        w = rng.standard_normal((N, 3)).astype(np.float32)                      # Cs = 2, M = 2: CsEff = 1 last
        cases["n%d_k3_seeded" % N] = (w, 2, 3, 2, None, 3)
        cases["n%d_k5_given" % N] = (w[:, :1].copy(), 1, 5, 1, rng.standard_normal((1, 5, 1)).astype(np.float32), 2)
        w1 = rng.standard_normal((N, 1)).astype(np.float32)
        init = rng.standard_normal((1, 256, 1)).astype(np.float32)
        cases["n%d_k256_given" % N] = (w1, 1, 256, 1, init, 2 if N <= 257 else 1)
        if N <= 257 or N == 4097:
            cases["n%d_k256_seeded" % N] = (w1, 1, 256, 1, None, 2 if N <= 257 else 1)
    return cases


# ------------------------------------------------------------------------------ cs_sweep
def cs_sweep():
    """Every Cs from 1 to 16 with every CsEff from 1 to Cs in the last of two sub-spaces (CsEff = Cs: a full one); K = 2
    seeded and K = 11 with a given book whose padded dims are not zero.  Cs % 4 == 0 runs as a conv layer."""
    cases = {}
    for Cs in range(1, 17):
        for cse in range(1, Cs + 1):
            rng = np.random.default_rng(400 + 17 * Cs + cse)
            shape = (4, Cs + cse, 2, 3) if Cs % 4 == 0 else (23, Cs + cse)
            w = rng.standard_normal(shape).astype(np.float32)
            cases["cs%d_eff%d_k2_seeded" % (Cs, cse)] = (w, 2, 2, Cs, None, 3)
            cases["cs%d_eff%d_k11_given" % (Cs, cse)] = (w, 2, 11, Cs, rng.standard_normal((2, 11, Cs)).astype(np.float32), 3)
    return cases


# ------------------------------------------------------------------------------ empty_words
MARKS = _bits(0x80000000, 0x00000001, 0x80000001, 0x4B7FABCD, 0xCB123456, 0x3F800001, 0x007FFFFF)   # -0.0 first


def _marked_book(P, M, K, Cs, cin, live):
    """[M][K][Cs]: the code words `live` are points of P [M][N][Cs]; every other entry holds one of MARKS (finite, far from
    the points, which sit around 10); the padded dims hold 7.5 + k."""
    book = np.empty((M, K, Cs), np.float32)
    for m in range(M):
        for k in range(K):
            for j in range(Cs):
                book[m, k, j] = MARKS[(m + 3 * k + j) % len(MARKS)]
        for i, k in enumerate(live):
            book[m, k] = P[m, (5 * i + m) % P.shape[1]]
        cse = min(cin - m * Cs, Cs)
        book[m, :, cse:] = 7.5 + np.arange(K)[:, None]
    return book


def empty_words():
    """Given books in which most code words attract no point and hold recognisable bits (-0.0, subnormals, odd mantissas),
    with padded dims that are not zero: the former come back untouched, the latter as +0.0."""
    cases = {}
    rng = np.random.default_rng(501)

    def pts(w, M, Cs):
        n, cin = w.shape
        pad = np.zeros((n, M * Cs), np.float32)
        pad[:, :cin] = w
        return pad.reshape(n, M, Cs).transpose(1, 0, 2)

    w = (rng.standard_normal((40, 7)) + 10.0).astype(np.float32)                # Cs = 4, CsEff = 3 last
    book = _marked_book(pts(w, 2, 4), 2, 256, 4, 7, (3, 77, 128, 200, 254, 255))
    cases["k256_n40_iter3"] = (w, 2, 256, 4, book, 3)
    cases["k256_n40_iter0"] = (w, 2, 256, 4, book, 0)
    w = (rng.standard_normal((100, 5)) + 10.0).astype(np.float32)               # Cs = 2, CsEff = 1 last
    cases["k16_m3_iter2"] = (w, 3, 16, 2, _marked_book(pts(w, 3, 2), 3, 16, 2, 5, (1, 14)), 2)
    return cases


# ------------------------------------------------------------------------------ range
def _diameter2(w, M, Cs):
    """Largest squared distance between two points of a sub-space (and where): no distance of a run exceeds it, since the
    code words are points or means of points."""
    best = (0.0, 0, 0, 0)
    cin = w.shape[1]
    for m in range(M):
        p = w[:, m * Cs:min(cin, (m + 1) * Cs)].astype(np.float64)
        d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        i, j = np.unravel_index(np.argmax(d), d.shape)
        if d[i, j] > best[0]:
            best = (float(d[i, j]), m, int(i), int(j))
    return best


def range_cases():
    """Unit-scale weights times a power of two: one that makes every squared distance fp32-subnormal or zero, and one that
    puts the largest squared distance within 2^4 of FLT_MAX, still finite.  One IEEE rounding per operation, subnormals kept."""
    cases = {}
    rng = np.random.default_rng(601)
    w = rng.standard_normal((150, 5)).astype(np.float32)                        # Cs = 3, CsEff = 2 last
    d2 = _diameter2(w, 2, 3)[0]
    small = w * np.float32(2.0 ** int(np.floor((-127.0 - np.log2(d2)) / 2)))     # diameter^2 <= 2^-127
    cases["subnormal_seeded"] = (small, 2, 4, 3, None, 3)
    cases["subnormal_given"] = (small, 2, 4, 3, _book([small[3:7, 0:3], small[8:12, 3:5]], 3), 3)
    w1 = w[:, :3].copy()
    d2, _, i, j = _diameter2(w1, 1, 3)
    w1[[0, i]] = w1[[i, 0]]                                                     # an end of the diameter is point 0 ...
    j = i if j == 0 else j
    large = w1 * np.float32(2.0 ** int(np.floor((127.5 - np.log2(d2)) / 2)))     # 2^125.5 < diameter^2 <= 2^127.5
    cases["near_flt_max_seeded"] = (large, 1, 4, 3, None, 3)                    # ... so round 1 of the seeding computes it
    cases["near_flt_max_given"] = (large, 1, 4, 3, _book([large[[0, j, 5, 6]]], 3), 3)
    return cases


# ------------------------------------------------------------------------------ active_set
def active_set():
    """Four sub-spaces with a given book: sub-space 0 is a fixed point from the start (every point is a code word), the
    others converge at different steps.  max_iter = 60 lets all of them converge, max_iter = 2 stops with some still moving."""
    rng = np.random.default_rng(701)
    N, K, Cs = 90, 4, 2
    book = rng.standard_normal((4, K, Cs)).astype(np.float32)
    subs = [book[0][np.arange(N) % K]]
    centres = rng.standard_normal((K, Cs)) * 8.0
    subs.append((centres[np.arange(N) % K] + 0.3 * rng.standard_normal((N, Cs))).astype(np.float32))   # four clear clusters
    subs += [rng.standard_normal((N, Cs)).astype(np.float32) for _ in range(2)]
    w = _fc(subs)
    return {"m4_iter60": (w, 4, K, Cs, book, 60), "m4_iter2": (w, 4, K, Cs, book, 2)}


FAMILIES = dict(ties_assign=ties_assign, ties_seed=ties_seed, sum_order=sum_order, sizes=sizes, cs_sweep=cs_sweep,
                empty_words=empty_words, range=range_cases, active_set=active_set)
