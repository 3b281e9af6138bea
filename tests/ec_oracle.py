"""TEST HELPER — numpy fp64 restatement of the error-corrected quantisation contract of qcnn_calib_gram /
qcnn_quantize_layer_ec (include/qcnn_hip.h, DESIGN.md "Error-corrected quantisation").

Patch index p = (y * kw + x) * Cg + c; block (y, x, m) = p in (y * kw + x) * Cg + m * Cs + [0, CsEff(m)).
J = sum_ct e_ct^T G_g(ct) e_ct with e = w - w_hat in patch order.  Replacing the code word of a block by c_cur + d moves
e by -d on that block: J changes by -2 d^T Hm[ct][b] + d^T G_bb d with Hm = E G.  Moving code word k by delta moves e by
-delta on every block that names k: J changes by -2 delta^T v_k + delta^T A_k delta, minimal at A_k delta = v_k.
"""
from __future__ import annotations

import numpy as np


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
    gbb = st.G[:, b, b][st.grp_of]                                       # [Ct][n][n]
    return -2.0 * np.einsum("ckj,cj->ck", d, st.Hm[:, b]) + np.einsum("cki,cij,ckj->ck", d, gbb, d)


def follow(st, d, b):
    """Hm after every channel's e moved by -d [Ct][n] on the index range b."""
    ctg = st.ct // st.grp
    for g in range(st.grp):
        st.Hm[g * ctg:(g + 1) * ctg] -= d[g * ctg:(g + 1) * ctg] @ st.G[g][b, :]


def assign_step(st, m, t):
    """Returns the number of assignments that changed."""
    b, n = st.block(t, m), st.cse(m)
    dl = deltas(st, m, t)
    best = np.argmin(dl, axis=1)                                         # lowest k of the minimum
    move = dl[np.arange(st.ct), best] < 0.0
    c = st.C[m, :, :n].astype(np.float64)
    new = np.where(move, best, st.A[:, t, m])
    d = c[new] - c[st.A[:, t, m]]                                        # [Ct][n], zero where nothing moves
    st.A[:, t, m] = new
    st.E[:, b] -= d
    follow(st, d, b)
    return int(move.sum())


def normal_equations(st, m, k):
    """A_k (without the ridge), v_k of code word k of sub-space m."""
    n = st.cse(m)
    A, v = np.zeros((n, n)), np.zeros(n)
    for ct, t in zip(*np.nonzero(st.A[:, :, m] == k)):
        bt = st.block(t, m)
        v += st.Hm[ct, bt]
        for t2 in np.nonzero(st.A[ct, :, m] == k)[0]:
            A += st.G[st.grp_of[ct]][bt, st.block(t2, m)]
    return A, v


def solve_words(st, m, ks):
    """delta of the code words ks from the CURRENT state (no interaction between them assumed); None = keeps its value."""
    n = st.cse(m)
    out = {}
    for k in ks:
        if not (st.A[:, :, m] == k).any():
            continue
        if st.taps == 1:                                                 # one block per channel: A_k = members per group x G_bb
            b, sel = st.block(0, m), st.A[:, 0, m] == k
            A = sum(np.count_nonzero(sel & (st.grp_of == g)) * st.G[g][b, b] for g in range(st.grp))
            v = st.Hm[sel, b].sum(axis=0)
        else:
            A, v = normal_equations(st, m, k)
        try:
            L = np.linalg.cholesky(A + st.lam * np.eye(n))
        except np.linalg.LinAlgError:
            continue
        out[k] = np.linalg.solve(L.T, np.linalg.solve(L, v))
    return out


def apply_words(st, m, dl):
    """c_k += delta (rounded to float32); E / Hm follow the code words as they were stored.  Returns code words that moved."""
    n, moved = st.cse(m), 0
    if st.taps == 1 and dl:
        b, d = st.block(0, m), np.zeros((st.K, n))
        for k, delta in dl.items():
            old = st.C[m, k, :n].astype(np.float64)
            st.C[m, k, :n] = (old + delta).astype(np.float32)
            d[k] = st.C[m, k, :n].astype(np.float64) - old
        dc = d[st.A[:, 0, m]]
        st.E[:, b] -= dc
        follow(st, dc, b)
        return int(np.count_nonzero(np.any(d != 0.0, axis=1)))
    for k, delta in dl.items():
        old = st.C[m, k, :n].astype(np.float64)
        st.C[m, k, :n] = (old + delta).astype(np.float32)
        d = st.C[m, k, :n].astype(np.float64) - old
        moved += int(np.any(d != 0.0))
        for ct, t in zip(*np.nonzero(st.A[:, :, m] == k)):
            bt = st.block(t, m)
            st.E[ct, bt] -= d
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


def sweep(st):
    """Returns (assignments changed, code words moved)."""
    changed = moved = 0
    for m in range(st.M):
        for t in range(st.taps):
            changed += assign_step(st, m, t)
        moved += update_step(st, m)
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
