"""TEST HELPER — numpy fp64 restatement of the error-corrected quantisation contract of qcnn_calib_gram /
qcnn_quantize_layer_ec (include/qcnn_hip.h, DESIGN.md "Error-corrected quantisation").

Patch index p = (y * kw + x) * Cg + c; block (y, x, m) = p in (y * kw + x) * Cg + m * Cs + [0, CsEff(m)).
J = sum_ct e_ct^T G_g(ct) e_ct with e = w - w_hat in patch order.  Replacing the code word of a block by c_cur + d moves
e by -d on that block: J changes by -2 d^T Hm[ct][b] + d^T G_bb d with Hm = E G.  Moving code word k by delta moves e by
-delta on every block that names k: J changes by -2 delta^T v_k + delta^T A_k delta, minimal at A_k delta = v_k.
"""
from __future__ import annotations

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53

# single mistakes the kernels could make, switched on in sweep(st, wrong=...): replay_sweep has to reject each of them on at least
# one case of tests/ec_cases.py (tests/test_ec_cases_cpu.py names which)
WRONG = ("taps_reversed",              # the taps of a sub-space in descending order
         "no_follow_between_taps",     # E follows every tap, Hm is refreshed only after the last tap of a sub-space
         "assign_le",                  # ties among improvements go to the highest k
         "move_on_zero",               # a move is taken at delta == 0
         "second_best",                # the second smallest delta wins
         "wave_low_only",              # argmin over k < 64: the cross-wave half of the reduction is lost
         "group0_gram",                # G[0] prices the blocks and forms A_k of every channel
         "update_one_shot",            # all K code words from one state on a multi-tap layer
         "update_stale_E",             # E follows a moved code word, Hm does not
         "empty_zero",                 # a code word without members becomes 0
         "nonpd_zero",                 # a code word whose A_k is not positive definite becomes 0
         "cseff_full",                 # the update works on Cs dims instead of CsEff (indices run on into the next tap)
         "members_last_dropped")       # the last member (highest ct * taps + t) of every code word is left out of A_k and v_k


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def patches(x_nhwc, grp, kh, kw, stride, pad):
    """[grp][rows][P] float64: every output pixel's input window per group, out-of-image taps zero."""
    x = np.asarray(x_nhwc, np.float64)
    n, H, W, C = x.shape
    cg = C // grp
    ho, wo = out_size(H, kh, stride, pad), out_size(W, kw, stride, pad)
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, C))
    xp[:, pad:pad + H, pad:pad + W] = x
    out = np.empty((grp, n, ho, wo, kh, kw, cg))
    for y in range(kh):
        for xx in range(kw):
            win = xp[:, y:y + (ho - 1) * stride + 1:stride, xx:xx + (wo - 1) * stride + 1:stride]
            for g in range(grp):
                out[g, :, :, :, y, xx] = win[..., g * cg:(g + 1) * cg]
    return out.reshape(grp, n * ho * wo, kh * kw * cg)


def gram(x_nhwc, grp, kh, kw, stride, pad):
    """[grp][P][P] float64 raw second moments; also returns sum |s_p s_q| (the scale of the error bound)."""
    s = patches(x_nhwc, grp, kh, kw, stride, pad)
    g = np.stack([a.T @ a for a in s])
    ga = np.stack([np.abs(a).T @ np.abs(a) for a in s])
    return g, ga


def dims(w):
    w = np.asarray(w)
    if w.ndim == 4:
        return w.shape
    return w.shape + (1, 1)


def to_patch_order(w):
    """[Ct][Cin][kh][kw] / [Ct][D] -> [Ct][P] float64, p = (y * kw + x) * Cin + c."""
    ct, cin, kh, kw = dims(w)
    return np.asarray(w, np.float64).reshape(ct, cin, kh, kw).transpose(0, 2, 3, 1).reshape(ct, kh * kw * cin)


def decode(ctrd, asmt, cin, taps):
    """w_hat [Ct][P] float64 from ctrd [M][K][Cs] and assignments [Ct][taps][M]."""
    ctrd = np.asarray(ctrd, np.float64)
    m, _, cs = ctrd.shape
    a = np.asarray(asmt).astype(np.intp).reshape(-1, taps, m)
    sub = ctrd[np.arange(m)[None, None, :], a]                           # [Ct][taps][M][Cs]
    return sub.reshape(a.shape[0], taps, m * cs)[..., :cin].reshape(a.shape[0], taps * cin)


class State:
    def __init__(self, w, ctrd, asmt, G, grp=1, ridge=0.0, lazy=False):
        self.ct, self.cin, kh, kw = dims(w)
        self.taps = kh * kw
        self.P = self.taps * self.cin
        self.grp = grp
        self.W = to_patch_order(w)
        self.C = np.array(ctrd, np.float32)
        self.M, self.K, self.Cs = self.C.shape
        self.A = np.array(asmt).astype(np.intp).reshape(self.ct, self.taps, self.M)
        self.G = np.broadcast_to(np.eye(self.P), (grp, self.P, self.P)) if G is None else np.asarray(G, np.float64)
        self.lam = ridge * float(np.mean([np.trace(g) for g in self.G])) / self.P
        self.grp_of = np.arange(self.ct) // (self.ct // grp)
        self.wrong = frozenset()                                         # mutation switches of sweep (WRONG); none: the contract
        if lazy:                                                         # E only: sweep_1x1 forms the columns of Hm it needs
            self.E, self.Hm = self.W - decode(self.C, self.A, self.cin, self.taps), None
        else:
            self.refresh()

    def cse(self, m):
        return min(self.cin - m * self.Cs, self.Cs)

    def block(self, t, m):
        b = t * self.cin + m * self.Cs
        return slice(b, b + self.cse(m))

    def refresh(self):
        self.E = self.W - decode(self.C, self.A, self.cin, self.taps)
        self.Hm = np.stack([self.E[i] @ self.G[self.grp_of[i]] for i in range(self.ct)]) if self.grp > 1 else self.E @ self.G[0]

    def objective(self):
        e = self.W - decode(self.C, self.A, self.cin, self.taps)
        ctg = self.ct // self.grp
        return float(sum(((e[g * ctg:(g + 1) * ctg] @ self.G[g]) * e[g * ctg:(g + 1) * ctg]).sum() for g in range(self.grp)))


def objective(w, ctrd, asmt, G, grp=1):
    return State(w, ctrd, asmt, G, grp).objective()


def deltas(st, m, t):
    """[Ct][K] float64: change of J when block (t, m) of channel ct takes code word k."""
    b, n = st.block(t, m), st.cse(m)
    c = st.C[m, :, :n].astype(np.float64)
    d = c[None, :, :] - c[st.A[:, t, m]][:, None, :]                     # [Ct][K][n]
    gbb = st.G[:, b, b][np.zeros_like(st.grp_of) if "group0_gram" in st.wrong else st.grp_of]          # [Ct][n][n]
    return -2.0 * np.einsum("ckj,cj->ck", d, st.Hm[:, b]) + np.einsum("cki,cij,ckj->ck", d, gbb, d)


def follow(st, d, b):
    """Hm after every channel's e moved by -d [Ct][n] on the index range b."""
    ctg = st.ct // st.grp
    for g in range(st.grp):
        st.Hm[g * ctg:(g + 1) * ctg] -= d[g * ctg:(g + 1) * ctg] @ st.G[g][b, :]


def pick(dl, cur, wrong=frozenset()):
    """The assign rule on deltas [Ct][K]: the lowest k of the smallest delta, taken only if that delta is < 0."""
    rows = np.arange(dl.shape[0])
    if "wave_low_only" in wrong:
        dl = dl[:, :64]
    if "second_best" in wrong:
        best = np.argsort(dl, axis=1, kind="stable")[:, 1]
    elif "assign_le" in wrong:
        best = dl.shape[1] - 1 - np.argmin(dl[:, ::-1], axis=1)
    else:
        best = np.argmin(dl, axis=1)                                     # lowest k of the minimum
    move = dl[rows, best] <= 0.0 if "move_on_zero" in wrong else dl[rows, best] < 0.0
    return np.where(move, best, cur)


def assign_step(st, m, t):
    """Returns the number of assignments that changed."""
    b, n = st.block(t, m), st.cse(m)
    cur = st.A[:, t, m].copy()
    new = pick(deltas(st, m, t), cur, st.wrong)
    c = st.C[m, :, :n].astype(np.float64)
    d = c[new] - c[cur]                                                  # [Ct][n], zero where nothing moves
    st.A[:, t, m] = new
    st.E[:, b] -= d
    if "no_follow_between_taps" not in st.wrong:
        follow(st, d, b)
    return int((new != cur).sum())


def members(st, m, k):
    """(ct, t) of the blocks of sub-space m that name code word k, ascending ct * taps + t."""
    mem = list(zip(*np.nonzero(st.A[:, :, m] == k)))
    return mem[:-1] if "members_last_dropped" in st.wrong else mem


def normal_equations(st, m, k):
    """A_k (without the ridge), v_k of code word k of sub-space m."""
    n = st.cse(m)
    idx = lambda t: np.arange(st.block(t, m).start, st.block(t, m).start + n)
    if "cseff_full" in st.wrong:
        n = st.Cs
        idx = lambda t: (t * st.cin + m * st.Cs + np.arange(n)) % st.P
    A, v = np.zeros((n, n)), np.zeros(n)
    mem = members(st, m, k)
    for ct, t in mem:
        bt = idx(t)
        v += st.Hm[ct, bt]
        g = 0 if "group0_gram" in st.wrong else st.grp_of[ct]
        for ct2, t2 in mem:
            if ct2 == ct:
                A += st.G[g][np.ix_(bt, idx(t2))]
    return A, v


def solve_words(st, m, ks):
    """delta of the code words ks from the CURRENT state (no interaction between them assumed); None = keeps its value."""
    out = {}
    plain = not st.wrong & {"members_last_dropped", "cseff_full", "group0_gram"}
    for k in ks:
        n = st.cse(m)
        zero = -st.C[m, k, :n].astype(np.float64)                        # the move that makes the word 0 (mutations only)
        if not members(st, m, k):
            if "empty_zero" in st.wrong:
                out[k] = zero
            continue
        if st.taps == 1 and plain:                                       # one block per channel: A_k = members per group x G_bb
            b, sel = st.block(0, m), st.A[:, 0, m] == k
            A = sum(np.count_nonzero(sel & (st.grp_of == g)) * st.G[g][b, b] for g in range(st.grp))
            v = st.Hm[sel, b].sum(axis=0)
        else:
            A, v = normal_equations(st, m, k)
        try:
            L = np.linalg.cholesky(A + st.lam * np.eye(len(v)))
        except np.linalg.LinAlgError:
            if "nonpd_zero" in st.wrong:
                out[k] = zero
            continue
        out[k] = np.linalg.solve(L.T, np.linalg.solve(L, v))
    return out


def store_word(st, m, k, delta):
    """c_k += delta, rounded to float32 once; returns the move as stored on the CsEff dims E and Hm follow."""
    n = st.cse(m)
    old = st.C[m, k, :n].astype(np.float64)
    st.C[m, k, :len(delta)] = (st.C[m, k, :len(delta)].astype(np.float64) + delta).astype(np.float32)
    return st.C[m, k, :n].astype(np.float64) - old


def apply_words(st, m, dl):
    """c_k += delta (rounded to float32); E / Hm follow the code words as they were stored.  Returns code words that moved."""
    n, moved = st.cse(m), 0
    stale = "update_stale_E" in st.wrong
    if st.taps == 1 and dl:
        b, d = st.block(0, m), np.zeros((st.K, n))
        for k, delta in dl.items():
            d[k] = store_word(st, m, k, delta)
        dc = d[st.A[:, 0, m]]
        st.E[:, b] -= dc
        if not stale:
            follow(st, dc, b)
        return int(np.count_nonzero(np.any(d != 0.0, axis=1)))
    for k, delta in dl.items():
        d = store_word(st, m, k, delta)
        moved += int(np.any(d != 0.0))
        for ct, t in zip(*np.nonzero(st.A[:, :, m] == k)):
            bt = st.block(t, m)
            st.E[ct, bt] -= d
            if not stale:
                st.Hm[ct] -= d @ st.G[st.grp_of[ct]][bt, :]
    return moved


def update_step(st, m, one_shot=None):
    """Sequential in k; for kh = kw = 1 (one_shot default) all K at once: code words that share no channel do not interact."""
    if one_shot is None:
        one_shot = st.taps == 1
    if one_shot:
        return apply_words(st, m, solve_words(st, m, range(st.K)))
    return sum(apply_words(st, m, solve_words(st, m, [k])) for k in range(st.K))


def sweep_1x1(st):
    """The sweep for kh = kw = 1 without a resident Hm: a sub-space step reads Hm only on its own block, and those columns are
    E G[:, b] of the moment (E is kept up to date), so each step costs one [Ct x P] x [P x CsEff] product instead of two passes
    over the whole of Hm.  Same formulas, same order, same results as assign_step + update_step to fp64 rounding
    (tests/test_ec_oracle_cpu.py); st.Hm is left unset."""
    changed = moved = 0
    ctg, rows = st.ct // st.grp, np.arange(st.ct)
    for m in range(st.M):
        b, n = st.block(0, m), st.cse(m)
        h = np.concatenate([st.E[g * ctg:(g + 1) * ctg] @ np.ascontiguousarray(st.G[g][:, b]) for g in range(st.grp)])
        gbb = st.G[:, b, b]
        gct = gbb[st.grp_of]
        c = st.C[m, :, :n].astype(np.float64)
        cur = st.A[:, 0, m]
        d = c[None, :, :] - c[cur][:, None, :]
        dl = -2.0 * np.einsum("ckj,cj->ck", d, h) + np.einsum("cki,cij,ckj->ck", d, gct, d)
        best = np.argmin(dl, axis=1)
        move = dl[rows, best] < 0.0
        new = np.where(move, best, cur)
        ds = c[new] - c[cur]
        st.A[:, 0, m] = new
        st.E[:, b] -= ds
        h -= np.einsum("ci,cij->cj", ds, gct)
        changed += int(move.sum())
        dk = np.zeros((st.K, n))
        for k in range(st.K):
            sel = new == k
            if not sel.any():
                continue
            A = sum(np.count_nonzero(sel & (st.grp_of == g)) * gbb[g] for g in range(st.grp)) + st.lam * np.eye(n)
            try:
                L = np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                continue
            delta = np.linalg.solve(L.T, np.linalg.solve(L, h[sel].sum(axis=0)))
            st.C[m, k, :n] = (c[k] + delta).astype(np.float32)
            dk[k] = st.C[m, k, :n].astype(np.float64) - c[k]
        st.E[:, b] -= dk[new]
        moved += int(np.count_nonzero(np.any(dk != 0.0, axis=1)))
    st.Hm = None
    return changed, moved


def sweep(st, wrong=()):
    """Returns (assignments changed, code words moved).  wrong: switches of WRONG, single mistakes for replay_sweep to reject."""
    assert all(x in WRONG for x in wrong), wrong
    st.wrong = frozenset(wrong)
    changed = moved = 0
    for m in range(st.M):
        for t in (reversed(range(st.taps)) if "taps_reversed" in st.wrong else range(st.taps)):
            changed += assign_step(st, m, t)
        if "no_follow_between_taps" in st.wrong:
            st.refresh()
        moved += update_step(st, m, one_shot=True if "update_one_shot" in st.wrong else None)
    st.wrong = frozenset()
    return changed, moved


def quantize_layer_ec(w, ctrd, asmt, G, grp=1, sweeps=4, ridge=1e-6):
    """(ctrd, asmt in the shape given, obj_trace [sweeps + 1], changed [sweeps]) of the contract, all fp64."""
    fc = dims(w)[2] * dims(w)[3] == 1
    st = State(w, ctrd, asmt, G, grp, ridge, lazy=fc)
    obj, chg, moved = [st.objective()], [], 1
    for _ in range(sweeps):
        if chg and chg[-1] == 0 and moved == 0:
            obj.append(obj[-1]); chg.append(0)
            continue
        if fc:
            c, moved = sweep_1x1(st)
        else:
            st.refresh()
            c, moved = sweep(st)
        chg.append(c)
        obj.append(st.objective())
    return st.C, st.A.astype(np.uint8).reshape(np.shape(asmt)), np.array(obj), np.array(chg)


# ------------------------------------------------------------------------------ replaying one sweep step by step
class ReplayError(AssertionError):
    """A step of the contract that the returned book / assignments cannot have come from; where = (m, t, ct) or (m, k)."""

    def __init__(self, where, what):
        super().__init__("%s: %s" % (where, what))
        self.where = where


CLEAR = 1e3     # a decision is clear when the runner-up is CLEAR tolerances away: a code word rounded differently to fp32 moves a
                # delta by 2^-24 relative at most, 2^29 tolerances of the fp64 pricing; anything nearer than that is a near-tie


def assign_tolerance(st, m, t):
    """[Ct] rounding bound of one delta priced in fp64: u64 x its n^2 + 2 n products x the largest sum of their magnitudes."""
    b, n = st.block(t, m), st.cse(m)
    c = st.C[m, :, :n].astype(np.float64)
    d = np.abs(c[None, :, :] - c[st.A[:, t, m]][:, None, :])
    gbb = np.abs(st.G[:, b, b][st.grp_of])
    mag = 2.0 * np.einsum("ckj,cj->ck", d, np.abs(st.Hm[:, b])) + np.einsum("cki,cij,ckj->ck", d, gbb, d)
    return U64 * (n * n + 2 * n) * mag.max(axis=1)


def replay_sweep(w, ctrd0, asmt0, G, grp, ridge, ctrd1, asmt1):
    """Checks every step of ONE sweep of the contract (sweeps = 1: start ctrd0 / asmt0, result ctrd1 / asmt1) against the fp64
    state, adopting the returned value after each check so that a near-tie decided differently cannot send the two runs apart.
    Within one sweep the assignments of sub-space m change only in m's assign phase and its code words only in m's update, so
    asmt1[:, :, m] and ctrd1[m] are the values of those moments.

    Assign step (m, t), tol = assign_tolerance, best = min(min_k delta, 0): a channel that moved has delta_chosen < tol and
    <= best + tol, one that stayed has best >= -tol.  Code words of equal value are one alternative (their deltas are the same
    number); where the runner-up alternative is at least CLEAR * tol away the decision is clear and the returned assignment
    must be the contract's: the lowest k of the best alternative if its delta is < 0, no move otherwise.

    Update of m, code word by code word in ascending k (all from one state for taps == 1): without members, or with an
    A_k + lambda I that Cholesky refuses, the word keeps its bits; otherwise |A delta - v| <= |A| u32 |c_new| (the word is
    stored in fp32) + u64 (terms of A_k + n) (|A| |delta| + sum |Hm members|) (fp64 sums in another order), A taken as the sum
    of |G| blocks.  Dims >= CsEff are +0.0.

    Returns dict(assign, update: worst figure / bound, gap: smallest gap / tol, clear, unclear: decisions, changed: assignments
    that differ from the start, solved, kept: code words).  Raises ReplayError at the first violation."""
    c0 = np.array(ctrd0, np.float32)
    cin = dims(w)[1]
    for m in range(c0.shape[0]):
        c0[m, :, max(0, min(cin - m * c0.shape[2], c0.shape[2])):] = 0.0                # the driver zeroes the padded dims
    st = State(w, c0, asmt0, G, grp, ridge)
    c1 = np.asarray(ctrd1, np.float32).reshape(st.C.shape)
    a1 = np.asarray(asmt1).astype(np.intp).reshape(st.A.shape)
    if not np.isfinite(c1).all():
        raise ReplayError((), "the returned book is not finite")
    if a1.min() < 0 or a1.max() >= st.K:
        raise ReplayError((), "a returned assignment is outside [0, K)")
    out = dict(assign=0.0, update=0.0, gap=np.inf, clear=0, unclear=0, changed=0, solved=0, kept=0)
    rows = np.arange(st.ct)
    for m in range(st.M):
        n = st.cse(m)
        for t in range(st.taps):
            b = st.block(t, m)
            dl, tol = deltas(st, m, t), assign_tolerance(st, m, t)
            cur, ret = st.A[:, t, m].copy(), a1[:, t, m]
            c = st.C[m, :, :n].astype(np.float64)
            best = np.minimum(dl.min(axis=1), 0.0)
            chosen = dl[rows, ret]
            for ct in range(st.ct):
                where = (m, t, ct)
                if ret[ct] != cur[ct]:
                    if not (chosen[ct] < tol[ct] and chosen[ct] <= best[ct] + tol[ct]):
                        raise ReplayError(where, "moved %d -> %d at delta %.17g, best %.17g (k = %d), tolerance %.3g"
                                          % (cur[ct], ret[ct], chosen[ct], best[ct], int(np.argmin(dl[ct])), tol[ct]))
                    fig = max(chosen[ct], chosen[ct] - best[ct])
                else:
                    if not best[ct] >= -tol[ct]:
                        raise ReplayError(where, "stayed at %d although k = %d lowers J by %.17g, tolerance %.3g"
                                          % (cur[ct], int(np.argmin(dl[ct])), -best[ct], tol[ct]))
                    fig = -best[ct]
                if tol[ct] > 0.0:
                    out["assign"] = max(out["assign"], fig / tol[ct])
                # alternatives: code words of equal value share one delta; "stay" is that of the current word, at 0
                same = np.all(c == c[cur[ct]], axis=1)
                alt = np.where(same, 0.0, dl[ct])                        # copies of the current word: d = 0 exactly
                lead = int(np.argmin(alt))
                if alt[lead] < 0.0:
                    tied = np.all(c == c[lead], axis=1)                  # the best alternative: every k that holds its value
                    gap = alt[~tied].min() - alt[lead]                   # "stay" is among the others, at 0
                    want = int(np.nonzero(tied)[0][0])                   # the lowest k among the improvements of that value
                else:                                                    # nothing improves: the best alternative is "stay"
                    gap = alt[~same].min() if not same.all() else np.inf
                    want = cur[ct]
                if tol[ct] > 0.0:
                    out["gap"] = min(out["gap"], gap / tol[ct])
                if gap >= CLEAR * tol[ct]:
                    out["clear"] += 1
                    if ret[ct] != want:
                        raise ReplayError(where, "clear decision (gap %.3g, tolerance %.3g): the contract takes %d, returned %d"
                                          % (gap, tol[ct], want, ret[ct]))
                else:
                    out["unclear"] += 1
            d = c[ret] - c[cur]
            st.A[:, t, m] = ret
            st.E[:, b] -= d
            follow(st, d, b)
            out["changed"] += int((ret != cur).sum())
        if c1[m, :, n:].tobytes() != np.zeros((st.K, st.Cs - n), np.float32).tobytes():
            raise ReplayError((m, int(np.nonzero(c1[m, :, n:].view(np.uint32).any(axis=1))[0][0])), "dims >= CsEff are not +0.0")

        def check(k):
            """The returned word k against the normal equations of the current state; returns its move or None (kept)."""
            mem = members(st, m, k)
            A, v = normal_equations(st, m, k)
            ok = bool(mem)
            if ok:
                try:
                    np.linalg.cholesky(A + st.lam * np.eye(n))
                except np.linalg.LinAlgError:
                    ok = False
            old, new = st.C[m, k, :n], c1[m, k, :n]
            if not ok:
                if new.tobytes() != old.tobytes():
                    raise ReplayError((m, k), "a code word %s must keep its bits: %r -> %r"
                                      % ("without members" if not mem else "whose A_k is not positive definite", old, new))
                out["kept"] += 1
                return None
            delta = new.astype(np.float64) - old.astype(np.float64)
            Aabs, hsum, terms = np.zeros((n, n)), np.zeros(n), 0
            for ct, t in mem:
                hsum += np.abs(st.Hm[ct, st.block(t, m)])
                for ct2, t2 in mem:
                    if ct2 == ct:
                        Aabs += np.abs(st.G[st.grp_of[ct]][st.block(t, m), st.block(t2, m)])
                        terms += 1
            Aabs += st.lam * np.eye(n)
            res = np.abs((A + st.lam * np.eye(n)) @ delta - v)
            bound = Aabs @ (U32 * np.abs(new.astype(np.float64))) + U64 * (terms + n) * (Aabs @ np.abs(delta) + hsum)
            ratio = np.where(bound > 0.0, res / np.where(bound > 0.0, bound, 1.0), np.where(res > 0.0, np.inf, 0.0))
            if not (res <= bound).all():
                raise ReplayError((m, k), "residual |A delta - v| = %r above its bound %r (%d members)" % (res, bound, len(mem)))
            out["update"] = max(out["update"], float(ratio.max()))
            out["solved"] += 1
            return delta

        def adopt(k, delta):
            st.C[m, k, :n] = c1[m, k, :n]
            for ct, t in members(st, m, k):
                bt = st.block(t, m)
                st.E[ct, bt] -= delta
                st.Hm[ct] -= delta @ st.G[st.grp_of[ct]][bt, :]

        if st.taps == 1:                                                 # all K from one state
            moves = [(k, check(k)) for k in range(st.K)]
            for k, delta in moves:
                if delta is not None:
                    adopt(k, delta)
        else:
            for k in range(st.K):
                delta = check(k)
                if delta is not None:
                    adopt(k, delta)
    assert np.array_equal(st.A, a1) and st.C.tobytes() == c1.tobytes()
    return out
