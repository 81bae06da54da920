"""The resumed capped walk — cursors under caps (miner_rank_topk_resume, miner_walk_advance;
corpus.WalkState / start_walk / advance_walk, rank_topk / rank_corpus with resume=,
corpus.rank_topk_deep_capped) — needs an MI355X.

The resumed form is never its own yardstick:
* A, exact: the numpy walk over S_gpu [U, N] of the UNCAPPED ranking kernels (base.world): chains of
  pages must concatenate to capt.capped_lists at full depth (per user ti.expected_lists under
  interest caps), and a page from a hand-made state must equal ``walk_from`` below — the same lexsort
  of the filters' survivors, cut strictly after the cursor, walked with the state's counts. Ids
  equal, scores bit for bit.
* B: capt.check_b / ti.check_b, the oracle's bar on every listed score.
* C: the capped call without ``resume`` (the form that was there before), bit for bit.
The worlds and cluster tables are those of tests/test_gpu_corpus_cap.py and
tests/test_gpu_corpus_interest.py (repeated rows as clusters of their own, n % 7 clusters in every
step, a contiguous block, unclustered rows, cluster id 2^31 - 1).
"""
import collections

import numpy as np
import pytest
import torch

import test_gpu_corpus_bias as biased
import test_gpu_corpus_cap as capt
import test_gpu_corpus_interest as ti
import test_gpu_corpus_rankof as base
from miner_amd import _lib, corpus

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:rank_topk. topk=:RuntimeWarning")]
DEV = base.DEV
DUP = base.DUP
BIG = 2 ** 31 - 1
INF = float("inf")
bits = base.bits
PAGES = (1, 7, 64, 100, 256)


def walk_from(S, keep, groups, cap, topk, cursors, used):
    """Yardstick A from a state: per user the lexsort of the survivors, the entries strictly after
    cursors[u] = (score, id), the greedy cap started at used[u] (a dict group -> count), the first
    topk, then the tail. ``groups``: int [N] (a cluster table) or [U, N] (per-user interests)."""
    U, N = S.shape
    Snp, g = S.numpy(), np.asarray(groups, np.int64)
    es = torch.full((U, topk), -INF)
    ei = torch.full((U, topk), -1, dtype=torch.int32)
    for u in range(U):
        gu = g if g.ndim == 1 else g[u]
        cs, ci = np.float32(cursors[u][0]), int(cursors[u][1])
        ids = np.flatnonzero(keep[u] & ~np.isnan(Snp[u]))
        order = ids[np.lexsort((ids, -Snp[u, ids].astype(np.float64)))]
        cnt, kept = dict(used[u]), []
        for n in order:
            s = Snp[u, n]
            if not (s < cs or (s == cs and n > ci)):          # a NaN cursor: never
                continue
            c = int(gu[n]) if n < len(gu) else -1
            if c >= 0:
                if max(cnt.get(c, 0), 0) >= cap:
                    continue
                cnt[c] = max(cnt.get(c, 0), 0) + 1
            kept.append(int(n))
            if len(kept) == topk:
                break
        if kept:
            idx = torch.tensor(kept)
            es[u, :len(kept)] = S[u, idx]
            ei[u, :len(kept)] = idx.int()
    return es, ei


def make_state(cursors, used, Q=corpus.MAX_WALK_GROUPS):
    """A hand-made WalkState on the device: used[u] a dict group -> count (sorted here)."""
    U = len(cursors)
    g = torch.zeros(U, Q, dtype=torch.int32)
    c = torch.zeros(U, Q, dtype=torch.int32)
    n = torch.zeros(U, dtype=torch.int32)
    for u, d in enumerate(used):
        keys = sorted(d)
        n[u] = len(keys)
        g[u, :len(keys)] = torch.tensor(keys, dtype=torch.int64).int()
        c[u, :len(keys)] = torch.tensor([d[k] for k in keys], dtype=torch.int64).int()
    return corpus.WalkState(torch.tensor([float(s) for s, _ in cursors], dtype=torch.float32).to(DEV),
                            torch.tensor([int(i) for _, i in cursors], dtype=torch.int64).int().to(DEV), g.to(DEV), c.to(DEV),
                            n.to(DEV), torch.zeros(U, dtype=torch.uint8, device=DEV))


def eq(got, want, what):
    gs, gi = got[0].cpu(), got[1].cpu()
    assert gi.dtype == torch.int32 and gs.dtype == torch.float32 and gs.shape == want[0].shape, what
    assert torch.equal(gi, want[1]), (what, np.argwhere((gi != want[1]).numpy())[:5].tolist())
    assert torch.equal(bits(gs), bits(want[0])), what


def chain(z, page, score_type, kw, capkw, clus_dev=None, limit=4000, pages=None):
    """Pages of ``page`` entries chained with advance_walk from the empty state until every row is
    short (``pages``: exactly that many); the concatenation on the CPU (pairs, or triples under
    interest caps)."""
    state = corpus.start_walk(z["U"], DEV)
    triple = "interest_cap" in capkw
    parts = []
    for _ in range(limit):
        got = corpus.rank_topk(z["m"], z["p"], z["t"], page, score_type=score_type, resume=state, **kw, **capkw)
        parts.append(got)
        if len(parts) == pages or (pages is None and bool((got[1][:, -1] < 0).all())):
            break
        state = corpus.advance_walk(state, got, news_cluster=None if triple else clus_dev)
    else:
        raise AssertionError("the walk did not end")
    assert not bool(state.overflow.any())
    return tuple(torch.cat([p[j] for p in parts], dim=1).cpu() for j in range(3 if triple else 2))


def test_the_new_surface_exists():
    for name in ("miner_rank_topk_resume", "miner_walk_advance"):
        assert hasattr(_lib.lib(), name)
    for name in ("WalkState", "start_walk", "advance_walk", "rank_topk_deep_capped"):
        assert hasattr(corpus, name)


CHAIN_CASES = [(s, t) for s in ("small_f32", "mid_f16", "mid_f32") for t in ("weighted", "max")]


@pytest.mark.parametrize("shape,score_type", CHAIN_CASES)
def test_chains_equal_the_walk(shape, score_type):
    """Caps 1, 2, 3 x pages of 1, 7, 64, 100, 256: the concatenation is capped_lists at full depth (A)
    and meets the oracle's bar (B); four pages of 64 are the capped top-256 (C); the empty state is
    the call without resume (C)."""
    z = capt.world(shape, score_type)
    U, N, clus = z["U"], z["N"], z["clus"]
    cd = clus.to(DEV)
    keep = base.keep_mask(U, N)
    for cap in (1, 2, 3):
        capkw = capt.caps_kw(clus, cap)
        for page in PAGES:
            got = chain(z, page, score_type, {}, capkw, cd)
            depth = got[0].shape[1]
            eq(got, capt.capped_lists(z["S"], keep, clus, cap, depth), (cap, page))
            assert depth >= page and (got[1][:, -1] < 0).all()
            capt.check_b(got, z["ref"], z["tol"], clus, cap, (cap, page))
        plain = corpus.rank_topk(z["m"], z["p"], z["t"], 256, score_type=score_type, **capkw)
        four = chain(z, 64, score_type, {}, capkw, cd, pages=4)
        assert torch.equal(four[1][:, :256], plain[1].cpu()) and torch.equal(bits(four[0][:, :256]), bits(plain[0].cpu())), cap
        for topk in (10, 100):
            a = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type, **capkw)
            b = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type, resume=corpus.start_walk(U, DEV), **capkw)
            c = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type, resume=corpus.start_walk(U, DEV, 0), **capkw)
            assert ti.same(a, b) and ti.same(a, c), (cap, topk)


@pytest.mark.parametrize("shape", ["small_f32", "mid_f16", "mid_f32"])
def test_chains_under_filters_subsets_and_priors(shape):
    """Once per shape: exclude_ids + eligible, news_ids (shuffled, with out-of-range ids), the G = 3 prior."""
    z = capt.world(shape, "weighted")
    U, N, clus = z["U"], z["N"], z["clus"]
    cd = clus.to(DEV)
    gen = torch.Generator().manual_seed(5 * N + U)
    sub, inside = biased.subset_ids(gen, N)
    pb = z["bias"][z["group"]].double().numpy()
    combos = [
        ("filters", dict(exclude_ids=z["hist"].to(DEV), eligible=z["ok"].to(DEV)), z["S"], None,
         base.keep_mask(U, N, z["hist"].numpy(), z["ok"].numpy())),
        ("subset", dict(news_ids=sub.to(DEV)), z["S"], None, base.keep_mask(U, N) & inside[None, :]),
        ("prior", biased.prior_kw(z), z["Sb"], pb, base.keep_mask(U, N)),
    ]
    for name, kw, S, prior, keep in combos:
        for cap, page in ((1, 7), (2, 64), (3, 100)):
            got = chain(z, page, "weighted", kw, capt.caps_kw(clus, cap), cd)
            eq(got, capt.capped_lists(S, keep, clus, cap, got[0].shape[1]), (name, cap, page))
            capt.check_b(got, z["ref"], z["tol"], clus, cap, (name, cap, page), prior)


@pytest.mark.parametrize("shape", ["small_f32", "mid_f16"])
def test_quota_only(shape):
    """A hand-made state at (+inf, -1): a cluster at cap, one at cap - 1, one absent, the repeated
    rows' pair clusters, cluster 2^31 - 1 as the table's last pair, a negative count."""
    z = capt.world(shape, "weighted")
    U, N, clus = z["U"], z["N"], z["clus"]
    keep = base.keep_mask(U, N)
    for cap in (1, 2, 3):
        used = []
        for u in range(U):
            d = {0: cap, 1: cap - 1, 3: -4, 5000: cap, BIG: cap if u % 2 else cap - 1}   # cluster 2 absent
            d.update({1000 + n: (cap if (n + u) % 2 else cap - 1) for n in range(DUP)})
            used.append(d)
        cursors = [(INF, -1)] * U
        for topk in (10, 100, 256):
            got = corpus.rank_topk(z["m"], z["p"], z["t"], topk, resume=make_state(cursors, used), **capt.caps_kw(clus, cap))
            want = walk_from(z["S"], keep, clus, cap, topk, cursors, used)
            eq(got, want, (cap, topk))
            capt.check_b(got, z["ref"], z["tol"], clus, cap, (cap, topk))
            listed = clus[want[1].clamp(min=0).long()][want[1] >= 0]
            assert not ((listed == 0) | (listed == 5000)).any()      # saturated clusters list nothing


@pytest.mark.parametrize("shape", ["small_f32", "mid_f16"])
def test_cursor_positions(shape):
    z = capt.world(shape, "weighted")
    U, N, clus, S = z["U"], z["N"], z["clus"], z["S"]
    excl, ok = z["hist"], z["ok"]
    keep = base.keep_mask(U, N, excl.numpy(), ok.numpy())
    fkw = dict(exclude_ids=excl.to(DEV), eligible=ok.to(DEV))
    used = [{0: 1, 2: 1, 6: 1, BIG: 1} for _ in range(U)]
    order = [np.lexsort((np.arange(N), -S[u].numpy().astype(np.float64))) for u in range(U)]
    bad = int(np.flatnonzero(~ok.numpy())[3])
    sets = {
        "an excluded news": [(float(S[u, int(excl[u, 20])]), int(excl[u, 20])) for u in range(U)],
        "an ineligible news": [(float(S[u, bad]), bad) for u in range(U)],
        "an id past N": [(float(S[u, order[u][30]]), N + 5) for u in range(U)],
        "a negative id": [(float(S[u, order[u][30]]), -1) for u in range(U)],
        "after everything": [(-INF, BIG)] * U,
        "nan": [(float("nan"), 0)] * U,
    }
    for cap in (1, 2):
        for name, cursors in sets.items():
            got = corpus.rank_topk(z["m"], z["p"], z["t"], 50, resume=make_state(cursors, used), **fkw, **capt.caps_kw(clus, cap))
            eq(got, walk_from(S, keep, clus, cap, 50, cursors, used), (name, cap))
            if name in ("after everything", "nan"):
                assert (got[1] == -1).all() and torch.isneginf(got[0]).all()
    # inside an exact tie of the repeated rows: the cursor is the lower id, the higher id is the very
    # next entry, and it appears or vanishes as its pair cluster's count says
    plain = base.keep_mask(U, N)
    for n in range(DUP):
        cursors = [(float(S[u, n]), n) for u in range(U)]
        for cnt, cap, there in ((1, 1, False), (1, 2, True), (0, 1, True), (2, 2, False)):
            state = make_state(cursors, [{3: 1, 1000 + n: cnt}] * U)
            got = corpus.rank_topk(z["m"], z["p"], z["t"], 20, resume=state, **capt.caps_kw(clus, cap))
            eq(got, walk_from(S, plain, clus, cap, 20, cursors, [{3: 1, 1000 + n: cnt}] * U), (n, cnt, cap))
            assert (got[1][:, 0] == N // 2 + n).all() == there and ((got[1] == N // 2 + n).any(dim=1)).all() == there
    # a cap changed between pages: cap 1, then cap 2 from the advanced state
    p1 = corpus.rank_topk(z["m"], z["p"], z["t"], 20, resume=corpus.start_walk(U, DEV), **capt.caps_kw(clus, 1))
    e1 = capt.capped_lists(S, plain, clus, 1, 20)
    eq(p1, e1, "page 1")
    state = corpus.advance_walk(corpus.start_walk(U, DEV), p1, news_cluster=clus.to(DEV))
    used = [dict(collections.Counter(int(clus[n]) for n in e1[1][u].tolist() if n >= 0 and clus[n] >= 0)) for u in range(U)]
    cursors = [(float(e1[0][u, -1]), int(e1[1][u, -1])) for u in range(U)]
    for cap, topk in ((2, 30), (1, 7), (3, 256)):
        got = corpus.rank_topk(z["m"], z["p"], z["t"], topk, resume=state, **capt.caps_kw(clus, cap))
        eq(got, walk_from(S, plain, clus, cap, topk, cursors, used), ("changed cap", cap))


@pytest.mark.parametrize("shape,score_type", [("mid_f16", "weighted"), ("mid_f16", "max"), ("k20_f16", "weighted")])
def test_interest_caps(shape, score_type):
    """Chains, four pages against the capped call, and the empty state under interest_cap 1, 2, 10 at
    K = 64 and K = 20, the interests returned with every page."""
    z = ti.world(shape, score_type)
    U, N, G = z["U"], z["N"], z["G"]
    keep = base.keep_mask(U, N)
    for icap in (1, 2, 10):
        capkw = dict(interest_cap=icap, return_interest=True)
        for page in PAGES:
            got = chain(z, page, score_type, {}, capkw)
            depth = got[0].shape[1]
            es, ei, eg = ti.expected_lists(z["S"], keep, G, icap, depth)
            eq(got, (es, ei), (icap, page))
            assert torch.equal(got[2], eg), (icap, page)
            ti.check_b(got, z["ref"], z["tol"], icap, (icap, page))
        plain = corpus.rank_topk(z["m"], z["p"], z["t"], 256, score_type=score_type, **capkw)
        four = chain(z, 64, score_type, {}, capkw, pages=4)
        assert ti.same(tuple(x[:, :256] for x in four), tuple(x.cpu() for x in plain)), icap
        a = corpus.rank_topk(z["m"], z["p"], z["t"], 100, score_type=score_type, **capkw)
        b = corpus.rank_topk(z["m"], z["p"], z["t"], 100, score_type=score_type, resume=corpus.start_walk(U, DEV, 64), **capkw)
        assert ti.same(a, b), icap
    # a hand-made quota under interest caps, with the filters
    keep = base.keep_mask(U, N, z["hist"].numpy(), z["ok"].numpy())
    used = [{k: (k + u) % 3 for k in range(0, z["K"], 2)} for u in range(U)]
    cursors = [(float(z["S"][u, 7 * u + 1]), 7 * u + 1) for u in range(U)]
    got = corpus.rank_topk(z["m"], z["p"], z["t"], 100, score_type=score_type, interest_cap=2, return_interest=True,
                           exclude_ids=z["hist"].to(DEV), eligible=z["ok"].to(DEV), resume=make_state(cursors, used, 64))
    want = walk_from(z["S"], keep, G.numpy(), 2, 100, cursors, used)
    eq(got, want, "interest quota")
    assert torch.equal(got[2].cpu(), torch.where(want[1] >= 0, torch.gather(G, 1, want[1].clamp(min=0).long()), -1).int())


def test_table_size_edges():
    """1,100 distinct clusters at N = 1,300 (d = 64, fp16, cap 1): n_used across 0, 1, 2, 3, 4, 1,023
    and 1,024 — the search's boundaries —, then capacity 8 and the overflow path."""
    U, K, d, N = 3, 32, 64, 1300
    m, p, t, gen = base.random_users(99, U, K, d, N, torch.float16, dup=DUP)
    S = base.gpu_score_matrix(m, p, t, "weighted")
    clus = torch.arange(N) % 1100
    clus[7::50] = -1
    keep = base.keep_mask(U, N)
    cursors = [(INF, -1)] * U
    for n_used in (0, 1, 2, 3, 4, 1023, 1024):
        used = [{int(c): 1 for c in torch.randperm(1100, generator=gen)[:n_used]} for _ in range(U)]
        if n_used:
            used[0] = {c: 1 for c in range(n_used)}                      # the lowest groups ...
            used[1] = {1099 - c: 1 for c in range(n_used)}               # ... and the highest
        state = make_state(cursors, used)
        assert state.n_used.tolist() == [n_used] * U
        got = corpus.rank_topk(m, p, t, 256, resume=state, news_cluster=clus.to(DEV), cluster_cap=1)
        eq(got, walk_from(S, keep, clus, 1, 256, cursors, used), n_used)
    # overflow: user 0's page holds 9 distinct clusters, the others' 3; capacity 8
    ids = torch.stack([torch.tensor([0, 1, 2, 3, 4, 5, 6, 8, 9]) if u == 0 else torch.tensor([0, 1, 2, 1100, 1101, 1102, 2, 1, 0]) for u in range(U)])
    page = (torch.gather(S, 1, ids).to(DEV), ids.int().to(DEV))
    state = corpus.advance_walk(corpus.start_walk(U, DEV, capacity=8), page, news_cluster=clus.to(DEV))
    assert state.capacity == 8 and state.overflow.tolist() == [1] + [0] * (U - 1)
    assert state.n_used.tolist() == [8] + [3] * (U - 1)
    assert float(state.scores[0]) == -INF and int(state.ids[0]) == BIG
    got = corpus.rank_topk(m, p, t, 100, resume=state, news_cluster=clus.to(DEV), cluster_cap=1)
    assert (got[1][0] == -1).all() and torch.isneginf(got[0][0]).all()
    cur = [(-INF, BIG)] + [(float(S[u, 0]), 0) for u in range(1, U)]
    used = [{}] + [{0: 2, 1: 2, 2: 2}] * (U - 1)
    eq(got, walk_from(S, keep, clus, 1, 100, cur, used), "after an overflow")
    again = corpus.advance_walk(state, got, news_cluster=clus.to(DEV))
    assert again.overflow.tolist()[0] == 1                               # an overflow stays set


def test_more_tiles_than_workgroups():
    """U = 515: 258 two-user tiles over at most 256 workgroups, every user with a state of its own —
    a workgroup's second tile must read its own users' tables."""
    U, K, d, N = 515, 32, 64, 600
    m, p, t, gen = base.random_users(U + N + 2, U, K, d, N, torch.float32, dup=DUP)
    S = base.gpu_score_matrix(m, p, t, "weighted")
    clus = capt.cluster_table(N)
    keep = base.keep_mask(U, N)
    order = np.argsort(-S.numpy(), axis=1, kind="stable")
    cursors, used = [], []
    for u in range(U):
        n = int(order[u, u % 50])
        cursors.append((float(S[u, n]), n))
        d_ = {(u + j) % 7: 2 for j in range(3)}
        if u % 3 == 0:
            d_[5000] = 1
        if u % 4 == 0:
            d_[BIG] = 2
        used.append(d_)
    got = corpus.rank_topk(m, p, t, 100, resume=make_state(cursors, used, 16), news_cluster=clus.to(DEV), cluster_cap=2)
    eq(got, walk_from(S, keep, clus, 2, 100, cursors, used), "515 users")


def test_rank_topk_deep_capped():
    z = capt.world("mid_f16", "weighted")
    U, N, clus = z["U"], z["N"], z["clus"]
    keep = base.keep_mask(U, N)
    out = corpus.rank_topk_deep_capped(z["m"], z["p"], z["t"], 600, return_state=True, **capt.caps_kw(clus, 2))
    assert len(out) == 3 and isinstance(out[2], corpus.WalkState) and not bool(out[2].overflow.any())
    want = capt.capped_lists(z["S"], keep, clus, 2, 650)
    eq(out[:2], (want[0][:, :600], want[1][:, :600]), "deep clusters")
    more = corpus.rank_topk(z["m"], z["p"], z["t"], 50, resume=out[2], **capt.caps_kw(clus, 2))
    eq(more, (want[0][:, 600:], want[1][:, 600:]), "one more page")
    assert ti.same(corpus.rank_topk_deep_capped(z["m"], z["p"], z["t"], 600, **capt.caps_kw(clus, 2)), out[:2])
    zi = ti.world("mid_f16", "weighted")
    got = corpus.rank_topk_deep_capped(zi["m"], zi["p"], zi["t"], 300, interest_cap=10, return_interest=True, return_state=True,
                                       exclude_ids=zi["hist"].to(DEV))
    keep = base.keep_mask(U, N, zi["hist"].numpy())
    es, ei, eg = ti.expected_lists(zi["S"], keep, zi["G"], 10, 340)
    eq(got[:2], (es[:, :300], ei[:, :300]), "deep interests")
    assert torch.equal(got[2].cpu(), eg[:, :300])
    more = corpus.rank_topk(zi["m"], zi["p"], zi["t"], 40, interest_cap=10, return_interest=True, resume=got[3],
                            exclude_ids=zi["hist"].to(DEV))
    eq(more[:2], (es[:, 300:], ei[:, 300:]), "one more page of interests")
    assert torch.equal(more[2].cpu(), eg[:, 300:])


def test_walk_advance_alone():
    """miner_walk_advance against collections.Counter: tails, unclustered entries, ids past n_cluster,
    groups given or looked up, repeats within a page, the union with an existing table."""
    gen = torch.Generator().manual_seed(4)
    U, nc = 7, 500
    clus = torch.randint(-2, 40, (nc,), generator=gen)
    clus[::9] = BIG
    for k in (1, 5, 64, 200, 256):
        ids = torch.randint(0, nc + 50, (U, k), generator=gen)          # some at or past n_cluster
        for u in range(U):
            ids[u, max(0, k - 2 * u):] = -1                               # tails of every length (user 0: full)
        scores = torch.randn(U, k, generator=gen)
        scores[1, -1] = -INF
        groups = torch.randint(-1, 64, (U, k), generator=gen)
        old = [dict(collections.Counter(torch.randint(0, 80, (3 * u,), generator=gen).tolist())) for u in range(U)]
        old[2][BIG] = 4
        old[3][5] = -3                                                    # a negative count reads as 0
        state = make_state([(1.0, 1)] * U, old, 300)
        for given in (False, True):
            page = (scores.to(DEV), ids.to(DEV), groups.to(DEV)) if given else (scores.to(DEV), ids.int().to(DEV))
            new = corpus.advance_walk(state, page, news_cluster=None if given else clus.to(DEV))
            cs, ci = corpus.page_cursor((scores, ids))
            assert torch.equal(bits(new.scores.cpu()), bits(cs)) and torch.equal(new.ids.cpu(), ci), (k, given)
            assert new.overflow.sum() == 0 and new.capacity == 300
            for u in range(U):
                want = collections.Counter({g: max(c, 0) for g, c in old[u].items()})
                for j in range(k):
                    n = int(ids[u, j])
                    g = -1 if n < 0 else int(groups[u, j]) if given else (int(clus[n]) if n < nc else -1)
                    if g >= 0:
                        want[g] += 1
                nu = int(new.n_used[u])
                gg, cc = new.groups[u, :nu].tolist(), new.counts[u, :nu].tolist()
                assert gg == sorted(want) and all(a < b for a, b in zip(gg, gg[1:])), (k, given, u)
                assert cc == [want[g] for g in gg], (k, given, u)


def test_rank_corpus_resume():
    """rank_corpus(resume=) with a host batch smaller than U equals rank_topk(resume=) on the encoded users."""
    gen = torch.Generator().manual_seed(23)
    U, L, K, d, Dc, N = 5, 40, 32, 64, 96, 300
    table = (torch.randn(N, d, generator=gen) / d ** 0.5).to(DEV)
    mask = (torch.arange(L)[None, :] >= torch.randint(0, L - 4, (U, 1), generator=gen)).to(DEV)
    hid = torch.randint(0, N, (U, L), generator=gen).int().to(DEV)
    pk = corpus.pack_encoder((torch.randn(Dc, d, generator=gen) / d ** 0.5).to(DEV), (torch.randn(K, Dc, generator=gen) * 0.3).to(DEV),
                             (torch.randn(d, d, generator=gen) / d ** 0.5).to(DEV), dtype=torch.float32)
    clus = capt.cluster_table(N)
    kw = capt.caps_kw(clus, 1)
    mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
    seen = torch.where(mask, hid, -1)
    S = base.gpu_score_matrix(mui, proj, table, "weighted")
    keep = base.keep_mask(U, N, seen.cpu().numpy())
    p1 = corpus.rank_corpus(table, hid, mask, pk, 30, batch=2, exclude_history=True, resume=corpus.start_walk(U, DEV), **kw)
    state = corpus.advance_walk(corpus.start_walk(U, DEV), p1, news_cluster=clus.to(DEV))
    a = corpus.rank_corpus(table, hid, mask, pk, 30, batch=2, exclude_history=True, resume=state, **kw)
    b = corpus.rank_corpus(table, hid, mask, pk, 30, batch=U + 3, exclude_history=True, resume=state, **kw)
    c = corpus.rank_topk(mui, proj, table, 30, exclude_ids=seen, resume=state, **kw)
    assert ti.same(a, b) and ti.same(a, c)
    want = capt.capped_lists(S, keep, clus, 1, 60)
    eq(p1, (want[0][:, :30], want[1][:, :30]), "page 1")
    eq(a, (want[0][:, 30:], want[1][:, 30:]), "page 2")
