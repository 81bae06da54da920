"""The diversity re-ranking (include/miner_diversify.h, corpus.diversify_topk) restated in float64.

``greedy`` is the definition itself, in numpy float64 on the inputs exactly as stored (an fp16 / bf16
table upcast, the fp32 scores upcast, lambda as the fp32 value the kernel receives). ``check`` is the
tolerance-aware verifier: it follows the KERNEL's own prefix, so that a near-tie the kernel resolved
the other way cannot cascade into every later step, and asks at each step that the kernel's pick is
within ``tol_obj`` of the float64 best.

The tolerance is derived, not tuned:
  tol_sim = (d + 8) · 2^-23. An fp32 accumulation of d exact products errs by at most d · 2^-24
            relative to |a||b| (Cauchy-Schwarz bounds the sum of |products|); that applies to G_pq,
            G_pp and G_qq, and the square roots halve the latter two: 2 · d · 2^-24 in all. The
            sqrt, the product and the divide add a few ulps: 8 · 2^-23.
  tol_obj = 2 · ((1 − λ) · tol_sim + 2^-22 · (λ · |rel| + 1)): the error of one objective — the
            similarity's, scaled, and a few fp32 roundings of terms no larger than λ|rel| + 1 —
            twice, because two objectives are compared. |rel| is the largest of the user's candidates.
"""
import numpy as np

NEG_INF = float("-inf")


def _np(x, dtype=None):
    """numpy view of a numpy array or a (CPU or device) torch tensor; bf16 / fp16 upcast exactly."""
    if hasattr(x, "detach"):
        x = x.detach().cpu()
        if x.is_floating_point() and x.element_size() < 4:
            x = x.float()
        x = x.numpy()
    x = np.asarray(x)
    return x if dtype is None else x.astype(dtype)


def tolerances(d, lam, rel_abs_max):
    lam = float(np.float32(lam))
    tol_sim = (d + 8) * 2.0 ** -23
    return tol_sim, 2.0 * ((1.0 - lam) * tol_sim + 2.0 ** -22 * (lam * rel_abs_max + 1.0))


def _user(scores, ids, table, lam, relevance):
    """Candidate mask [P], rel [P] float64, sim [P,P] float64 (rows / columns of non-candidates 0)."""
    P, N = scores.shape[0], table.shape[0]
    s64 = scores.astype(np.float64)
    cand = (ids >= 0) & (ids < N) & np.isfinite(s64)
    rel = np.zeros(P)
    if cand.any():
        if relevance == "score":
            rel[cand] = s64[cand]
        elif relevance == "minmax":
            lo, hi = s64[cand].min(), s64[cand].max()
            if hi != lo:
                rel[cand] = (s64[cand] - lo) / (hi - lo)
        else:
            raise ValueError(relevance)
    sim = np.zeros((P, P))
    idx = np.flatnonzero(cand)
    if len(idx):
        with np.errstate(all="ignore"):
            E = table[ids[idx]].astype(np.float64)
            G = E @ E.T
            n = np.sqrt(np.diagonal(G))
            q = G / (n[:, None] * n[None, :])
            q[~np.isfinite(q)] = 0.0
            zero = np.diagonal(G) == 0
            q[zero, :] = 0.0
            q[:, zero] = 0.0
        sim[np.ix_(idx, idx)] = q
    return cand, rel, sim


def greedy(scores, ids, table, topk, lam, relevance="minmax", stats=None):
    """The definition. scores [U,P] fp32, ids [U,P] integer, table [N,d]; returns numpy
    (out_scores [U,topk] fp32, out_ids [U,topk] int64, out_pos [U,topk] int64, out_obj [U,topk] float64),
    the tail (-inf, -1, -1, -inf). ``stats`` (a dict) receives 'ties': how many steps had two or more
    open candidates at the maximal objective (resolved to the lower position), and 'steps'."""
    scores, ids, table = _np(scores, np.float32), _np(ids, np.int64), _np(table)
    U, P = scores.shape
    lam = float(np.float32(lam))
    oml = float(np.float32(1.0) - np.float32(lam))
    out_s = np.full((U, topk), NEG_INF, np.float32)
    out_i = np.full((U, topk), -1, np.int64)
    out_p = np.full((U, topk), -1, np.int64)
    out_o = np.full((U, topk), NEG_INF, np.float64)
    ties = steps = 0
    for u in range(U):
        cand, rel, sim = _user(scores[u], ids[u], table, lam, relevance)
        open_ = cand.copy()
        m = np.zeros(P)
        for t in range(min(topk, int(cand.sum()))):
            obj = np.where(open_, lam * rel - oml * m, NEG_INF)
            p = int(np.argmax(obj))                      # the first maximum: the lower position
            ties += int((obj[open_] == obj[p]).sum() > 1)
            steps += 1
            out_s[u, t], out_i[u, t], out_p[u, t], out_o[u, t] = scores[u, p], ids[u, p], p, obj[p]
            open_[p] = False
            m = sim[:, p].copy() if t == 0 else np.maximum(m, sim[:, p])
    if stats is not None:
        stats.update(ties=ties, steps=steps)
    return out_s, out_i, out_p, out_o


def check(got, inputs, dtype=None):
    """got = (out_scores, out_ids, out_pos[, out_obj]) [U,topk] as the kernel returned them;
    inputs = (scores, ids, table, topk, lam, relevance); ``dtype`` names the table's format in the
    messages (the tolerance does not depend on it: the inputs are taken as stored). Raises
    AssertionError on the first violation; returns the largest (float64 best − pick's objective) /
    tol_obj seen, a figure to print."""
    scores, ids, table, topk, lam, relevance = inputs
    scores, ids, table = _np(scores, np.float32), _np(ids, np.int64), _np(table)
    gs, gi, gp = _np(got[0], np.float32), _np(got[1], np.int64), _np(got[2], np.int64)
    go = _np(got[3], np.float64) if len(got) > 3 and got[3] is not None else None
    U, P = scores.shape
    d = table.shape[1]
    assert gs.shape == gi.shape == gp.shape == (U, topk), (gs.shape, gi.shape, gp.shape, (U, topk))
    lam32 = float(np.float32(lam))
    oml = float(np.float32(1.0) - np.float32(lam))
    worst = 0.0
    for u in range(U):
        what = f"{dtype} user {u}"
        cand, rel, sim = _user(scores[u], ids[u], table, lam, relevance)
        n = min(topk, int(cand.sum()))
        pos = gp[u, :n]
        assert ((pos >= 0) & (pos < P)).all(), (what, "a listed position outside the pool", pos)
        assert len(set(pos.tolist())) == n, (what, "positions repeat")
        assert cand[pos].all(), (what, "a non-candidate is listed")
        assert (gp[u, n:] == -1).all() and (gi[u, n:] == -1).all() and np.isneginf(gs[u, n:]).all(), (what, "tail")
        assert np.array_equal(gs[u, :n].view(np.uint32), scores[u, pos].view(np.uint32)), (what, "score bits")
        assert np.array_equal(gi[u, :n], ids[u, pos]), (what, "ids")
        _, tol_obj = tolerances(d, lam, float(np.abs(rel[cand]).max()) if cand.any() else 0.0)
        open_ = cand.copy()
        m = np.zeros(P)
        for t in range(n):
            obj = np.where(open_, lam32 * rel - oml * m, NEG_INF)
            p = int(pos[t])
            gap = float(obj.max() - obj[p])
            worst = max(worst, gap / tol_obj)
            assert gap <= tol_obj, (what, f"step {t}: picked position {p} with objective {obj[p]!r}, "
                                          f"best {obj.max()!r} at {int(np.argmax(obj))}, tol {tol_obj!r}")
            if go is not None:
                assert abs(go[u, t] - obj[p]) <= tol_obj, (what, f"step {t}: out_obj {go[u, t]!r} vs {obj[p]!r}")
            open_[p] = False
            m = sim[:, p].copy() if t == 0 else np.maximum(m, sim[:, p])
    return worst
