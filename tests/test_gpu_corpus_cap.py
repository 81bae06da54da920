"""Per-cluster caps (miner_rank_topk_capped, miner_topk_merge_capped; corpus.rank_topk / rank_corpus /
merge_topk / update_topk with news_cluster= / cluster_cap=, corpus.cap_topk) — needs an MI355X.

The capped forms are never compared with themselves alone. Their yardsticks are
* A, exact: S_gpu [U, N] of the UNCAPPED ranking kernels (base.world / base.gpu_score_matrix), plus
  bias[group] in torch fp32 where a prior is used. The expected list is made on the CPU:
  numpy.lexsort((ids, -S[u])) over the filters' survivors (base.keep_mask), the greedy cap (keep an
  entry iff fewer than cap of its cluster were kept before it), the first topk, then (-inf, -1). Ids
  must be equal and scores bit for bit.
* B: every returned score within base's bar of oracle.corpus_oracle's score for that id (fp32
  1e-5·|ref| + 1e-5·rms, 16-bit 2e-4 / 2e-4; with a prior, the prior added in float64 and one fp32
  rounding of the sum, 2^-23·|sum|, allowed on top), no cluster more than cap times, the order
  non-increasing with ties by id.
The cluster tables make the uncapped answer wrong: base's tables repeat rows [0, 8) at
[N/2, N/2 + 8) and each pair is one cluster (with cap 1 the higher id vanishes although it ties
exactly); n % 7 clusters span every 256-news step; one cluster is a contiguous block inside a step;
some news are unclustered (negative entries); one cluster id is 2^31 - 1.
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_corpus_bias as biased
import test_gpu_corpus_rankof as base
from miner_amd import _lib, corpus

pytestmark = pytest.mark.gpu
DEV = base.DEV
DUP = base.DUP
EPS = 2.0 ** -23
bits = base.bits
BIG = 2 ** 31 - 1


def cluster_table(N):
    """int64 [N]: n % 7 everywhere (every step holds all seven), a contiguous block [40, 70) in one
    cluster, ten news in cluster 2^31 - 1, every fifth news unclustered (-1 or -7), and each repeated
    pair (n, N/2 + n), n < 8, a cluster of its own."""
    n = torch.arange(N)
    g = n % 7
    g[40:70] = 5000
    g[100:110] = BIG
    g[n % 5 == 3] = -1
    g[n % 10 == 8] = -7
    g[:DUP] = 1000 + torch.arange(DUP)
    g[N // 2:N // 2 + DUP] = 1000 + torch.arange(DUP)
    return g


@functools.lru_cache(maxsize=None)
def world(shape, score_type):
    """biased.world (base.world plus a G = 3 prior and both yardsticks with it) plus the cluster table."""
    z = dict(biased.world(shape, score_type))
    z["clus"] = cluster_table(z["N"])
    return z


def capped_lists(S, keep, clus, cap, topk):
    """Yardstick A: per user the lexsort of the survivors, the greedy cap, the first topk, the tail."""
    U, N = S.shape
    Snp, g = S.numpy(), np.asarray(clus, np.int64)
    es = torch.full((U, topk), float("-inf"))
    ei = torch.full((U, topk), -1, dtype=torch.int32)
    for u in range(U):
        ids = np.flatnonzero(keep[u] & ~np.isnan(Snp[u]))
        order = ids[np.lexsort((ids, -Snp[u, ids].astype(np.float64)))]
        used, kept = {}, []
        for n in order:
            c = int(g[n]) if n < len(g) else -1
            if c >= 0:
                if used.get(c, 0) >= cap:
                    continue
                used[c] = used.get(c, 0) + 1
            kept.append(int(n))
            if len(kept) == topk:
                break
        if kept:
            idx = torch.tensor(kept)
            es[u, :len(kept)] = S[u, idx]
            ei[u, :len(kept)] = idx.int()
    return es, ei


def check_a(got, S, keep, clus, cap, topk, what):
    es, ei = capped_lists(S, keep, clus, cap, topk)
    gs, gi = got[0].cpu(), got[1].cpu()
    assert gs.shape == (S.shape[0], topk) and gi.dtype == torch.int32 and gs.dtype == torch.float32
    assert torch.equal(gi, ei), (what, np.argwhere((gi != ei).numpy())[:5].tolist())
    assert torch.equal(bits(gs), bits(es)), what
    return es, ei


def check_b(got, ref, tol, clus, cap, what, prior=None):
    """Yardstick B; ``ref`` float64 [U, N] holds the oracle's scores, ``prior`` float64 [U, N] what
    the call adds to them (the bar is the unbiased score's, plus one fp32 rounding of the sum)."""
    gs, gi = got[0].cpu().double().numpy(), got[1].cpu().long().numpy()
    rms = float(np.sqrt(np.mean(ref ** 2)))
    add = np.zeros_like(ref) if prior is None else prior
    g = np.asarray(clus, np.int64)
    for u in range(gs.shape[0]):
        n = gi[u][gi[u] >= 0]
        s = gs[u][:len(n)]
        assert (gi[u][len(n):] == -1).all() and np.isneginf(gs[u][len(n):]).all(), what
        r = ref[u, n]
        bound = tol["rtol"] * np.abs(r) + tol["rms_floor"] * rms + EPS * np.abs(s)
        assert (np.abs(s - (r + add[u, n])) <= bound).all(), what
        c = g[n]
        if (c >= 0).any():
            assert np.unique(c[c >= 0], return_counts=True)[1].max() <= cap, what
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (n[:-1] < n[1:]))).all(), what


def caps_kw(clus, cap, dtype=torch.int64):
    return dict(news_cluster=clus.to(DEV, dtype), cluster_cap=cap)


def test_the_new_surface_exists():
    for name in ("miner_rank_topk_capped", "miner_topk_merge_capped"):
        assert hasattr(_lib.lib(), name)
    assert callable(corpus.cap_topk)


@pytest.mark.parametrize("shape,score_type", base.CASES)
def test_rank_topk_capped(shape, score_type, monkeypatch):
    """topk 10 and 100, caps 1, 2 and 7: alone, with each filter (exclusion lists; the bitmap as bool
    and packed), the 60 % subset with junk ids, the G = 3 prior with groups, and all together. The
    split switch must not change a capped list."""
    z = world(shape, score_type)
    U, N, clus = z["U"], z["N"], z["clus"]
    gen = torch.Generator().manual_seed(3 * N + U)
    sub, inside = biased.subset_ids(gen, N)
    excl, ok = z["hist"], z["ok"]
    pkw = biased.prior_kw(z)
    pb = z["bias"][z["group"]].double().numpy()
    combos = [
        ("alone", dict(), z["S"], None, base.keep_mask(U, N)),
        ("excl", dict(exclude_ids=excl.to(DEV)), z["S"], None, base.keep_mask(U, N, excl.numpy())),
        ("bitmap", dict(eligible=ok.to(DEV)), z["S"], None, base.keep_mask(U, N, None, ok.numpy())),
        ("packed", dict(eligible=corpus.pack_eligible(ok.to(DEV))), z["S"], None, base.keep_mask(U, N, None, ok.numpy())),
        ("subset", dict(news_ids=sub.to(DEV)), z["S"], None, base.keep_mask(U, N) & inside[None, :]),
        ("prior", dict(**pkw), z["Sb"], pb, base.keep_mask(U, N)),
        ("all", dict(exclude_ids=excl.to(DEV), eligible=ok.to(DEV), news_ids=sub.to(DEV), **pkw), z["Sb"], pb,
         base.keep_mask(U, N, excl.numpy(), ok.numpy()) & inside[None, :]),
    ]
    for name, kw, S, prior, keep in combos:
        for topk in (10, 100):
            for cap in (1, 2, 7):
                what = (name, topk, cap)
                got = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type, **kw, **caps_kw(clus, cap))
                es, ei = check_a(got, S, keep, clus, cap, topk, what)
                check_b(got, z["ref"], z["tol"], clus, cap, what, prior)
                if name == "alone" and topk == 100 and cap == 1:
                    # the cap changed the answer: the uncapped list differs for every user, and the
                    # second copy of a repeated row is gone wherever the first is listed
                    plain = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type)[1].cpu()
                    assert (plain != ei).any(dim=1).all()
                    for u in range(U):
                        listed = set(ei[u].tolist())
                        assert not any(n in listed and N // 2 + n in listed for n in range(DUP))
                        assert not any(N // 2 + n in listed for n in range(DUP))   # the lower id of a tie is the kept one
    with monkeypatch.context() as mp:
        mp.setenv("MINER_RK_SPLIT", "1")
        name, kw, S, prior, keep = combos[-1]
        got = corpus.rank_topk(z["m"], z["p"], z["t"], 100, score_type=score_type, **kw, **caps_kw(clus, 2, torch.int32))
        check_a(got, S, keep, clus, 2, 100, "split switch")


@pytest.mark.parametrize("shape", ["mid_f16", "c5_f16"])
@pytest.mark.parametrize("rising", [True, False])
def test_sorted_tables(shape, rising):
    """The same table with its rows ordered so that user 0's score rises with the id: every step then
    brings better news than the list holds, kept entries are evicted step after step, and a news
    rejected early for a full cluster stays rejected. The descending order too (after the first step
    user 0 stages nothing)."""
    z = world(shape, "weighted")
    U, N = z["U"], z["N"]
    order = torch.argsort(z["S"][0], descending=not rising, stable=True)
    t2 = z["t"][order.to(DEV)].contiguous()
    S2 = z["S"][:, order]                        # the scores of a row do not depend on where it stands
    ref2 = z["ref"][:, order.numpy()]
    clus = z["clus"]
    for topk, cap in ((10, 1), (100, 2), (100, 7)):
        got = corpus.rank_topk(z["m"], z["p"], t2, topk, **caps_kw(clus, cap))
        check_a(got, S2, base.keep_mask(U, N), clus, cap, topk, (rising, topk, cap))
        check_b(got, ref2, z["tol"], clus, cap, (rising, topk, cap))


@pytest.mark.parametrize("shape,score_type", [("small_f32", "weighted"), ("mid_f16", "weighted"), ("c5_bf16", "weighted")])
def test_no_op_caps(shape, score_type):
    """cap >= topk, all clusters negative, every news its own cluster: the uncapped list, bit for bit."""
    z = world(shape, score_type)
    N = z["N"]
    for kw in (dict(), dict(exclude_ids=z["hist"].to(DEV), eligible=z["ok"].to(DEV)), biased.prior_kw(z)):
        for topk in (10, 100):
            want = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type, **kw)
            for clus, cap in ((z["clus"], topk), (z["clus"], 256), (torch.full((N,), -3), 1),
                              (torch.arange(N) * 7 + 1, 1), (torch.randperm(N, generator=torch.Generator().manual_seed(1)), 1)):
                got = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type, **kw, **caps_kw(clus, cap))
                assert torch.equal(got[1], want[1]) and torch.equal(bits(got[0]), bits(want[0])), (topk, cap)


@pytest.mark.parametrize("shape", ["small_f32", "mid_f16"])
def test_degenerate_caps(shape):
    """3 clusters, cap 2, nothing unclustered, topk 100: six entries, then the tail. The list never
    fills, the threshold stays -inf and every step stages all its 256 news."""
    z = world(shape, "weighted")
    U, N = z["U"], z["N"]
    clus = torch.arange(N) % 3
    got = corpus.rank_topk(z["m"], z["p"], z["t"], 100, **caps_kw(clus, 2))
    es, ei = check_a(got, z["S"], base.keep_mask(U, N), clus, 2, 100, "degenerate")
    assert ((ei >= 0).sum(1) == 6).all()
    check_b(got, z["ref"], z["tol"], clus, 2, "degenerate")


@pytest.mark.parametrize("U", [515, 2])
def test_more_tiles_than_workgroups(U):
    """U = 515: 258 two-user tiles over at most 256 workgroups (a workgroup's second tile starts from
    an empty capped list); U = 2: one tile, where the uncapped call would take the split form."""
    K, d, N = 32, 64, 300
    m, p, t, gen = base.random_users(U + N + 1, U, K, d, N, torch.float32, dup=DUP)
    S = base.gpu_score_matrix(m, p, t, "weighted")
    clus = cluster_table(N)
    excl = torch.randint(-1, N, (U, 30), generator=gen)
    ok = torch.rand(N, generator=gen) < 0.7
    for cap in (1, 2):
        got = corpus.rank_topk(m, p, t, 100, **caps_kw(clus, cap))
        check_a(got, S, base.keep_mask(U, N), clus, cap, 100, ("plain", cap))
    got = corpus.rank_topk(m, p, t, 100, exclude_ids=excl.to(DEV), eligible=ok.to(DEV), **caps_kw(clus, 1))
    check_a(got, S, base.keep_mask(U, N, excl.numpy(), ok.numpy()), clus, 1, 100, "filtered")
    sub, inside = biased.subset_ids(gen, N)
    got = corpus.rank_topk(m, p, t, 100, news_ids=sub.to(DEV), **caps_kw(clus, 2))
    check_a(got, S, base.keep_mask(U, N) & inside[None, :], clus, 2, 100, "subset")


def test_one_chunk_per_step():
    """fp16 at d = 64: a step is one chunk, so every merge — and its load of the staged entries'
    cluster ids — sits between two consecutive chunk barriers."""
    U, K, d, N = 5, 32, 64, 600
    m, p, t, gen = base.random_users(65, U, K, d, N, torch.float16, dup=DUP)
    clus = cluster_table(N)
    sub, inside = biased.subset_ids(gen, N)
    bias = biased.make_prior(gen, N)
    group = torch.arange(U) % biased.G
    for st in ("weighted", "mean"):
        S = base.gpu_score_matrix(m, p, t, st)
        for topk, cap in ((10, 1), (100, 2), (100, 7)):
            check_a(corpus.rank_topk(m, p, t, topk, score_type=st, **caps_kw(clus, cap)), S, base.keep_mask(U, N), clus,
                    cap, topk, (st, topk, cap))
        check_a(corpus.rank_topk(m, p, t, 100, score_type=st, news_ids=sub.to(DEV), **caps_kw(clus, 1)), S,
                base.keep_mask(U, N) & inside[None, :], clus, 1, 100, (st, "subset"))
        check_a(corpus.rank_topk(m, p, t, 100, score_type=st, news_bias=bias.to(DEV), user_group=group.to(DEV),
                                 **caps_kw(clus, 1)), S + bias[group], base.keep_mask(U, N), clus, 1, 100, (st, "prior"))
        check_a(corpus.rank_topk(m, p, t, 100, score_type=st, **caps_kw(torch.arange(N) % 3, 2)), S, base.keep_mask(U, N),
                torch.arange(N) % 3, 2, 100, (st, "degenerate"))


@pytest.mark.parametrize("shape", ["small_f32", "mid_f16", "c5_f16"])
def test_merge_family(shape):
    """merge_topk(capped(A), capped(B), caps) == capped(A ∪ B) for a random disjoint split;
    cap_topk(rank_topk(topk=256))[:k] == the capped rank_topk wherever it fills k; update_topk under
    caps == the capped ranking of the union for fresh rows new to the list — each also with
    ``eligible``; unsorted inputs, ka = 0 and ids at or past n_cluster."""
    z = world(shape, "weighted")
    U, N, clus = z["U"], z["N"], z["clus"]
    m, p, t = z["m"], z["p"], z["t"]
    gen = torch.Generator().manual_seed(N + 17)
    perm = torch.randperm(N, generator=gen)
    A, B = perm[:N // 2].to(DEV), perm[N // 2:].to(DEV)
    inA = np.zeros(N, bool)
    inA[perm[:N // 2].numpy()] = True
    ok = z["ok"]
    for cap, k in ((1, 10), (2, 100), (7, 100)):
        kw = caps_kw(clus, cap)
        la = corpus.rank_topk(m, p, t, k, news_ids=A, **kw)
        lb = corpus.rank_topk(m, p, t, k, news_ids=B, **kw)
        check_a(la, z["S"], base.keep_mask(U, N) & inA[None, :], clus, cap, k, ("A", cap))
        check_a(corpus.merge_topk(la, lb, k, **kw), z["S"], base.keep_mask(U, N), clus, cap, k, ("merge", cap))
        # under a bitmap: lists ranked under it, merged under it (a list capped without it has already
        # given up the news that a now-ineligible one displaced: update_topk's documented caveat)
        laok = corpus.rank_topk(m, p, t, k, news_ids=A, eligible=ok.to(DEV), **kw)
        lbok = corpus.rank_topk(m, p, t, k, news_ids=B, eligible=ok.to(DEV), **kw)
        check_a(corpus.merge_topk(laok, lbok, k, eligible=ok.to(DEV), **kw), z["S"], base.keep_mask(U, N, None, ok.numpy()),
                clus, cap, k, ("merge eligible", cap))
        # unsorted rows: the same sets in another order
        sh = torch.randperm(k, generator=gen).to(DEV)
        check_a(corpus.merge_topk((la[0][:, sh], la[1][:, sh]), (lb[0][:, sh], lb[1][:, sh]), k, **kw), z["S"],
                base.keep_mask(U, N), clus, cap, k, ("merge unsorted", cap))
        # update_topk: A is served, B is new to it
        check_a(corpus.update_topk(la, m, p, t, B, **kw), z["S"], base.keep_mask(U, N), clus, cap, k, ("update", cap))
        check_a(corpus.update_topk(laok, m, p, t, B, eligible=ok.to(DEV), **kw), z["S"],
                base.keep_mask(U, N, None, ok.numpy()), clus, cap, k, ("update eligible", cap))
        # the post-hoc cap of an uncapped top-256 (ka = 0 inside cap_topk): prefix-exact
        for elig, keep in ((None, base.keep_mask(U, N)), (ok.to(DEV), base.keep_mask(U, N, None, ok.numpy()))):
            full = corpus.rank_topk(m, p, t, 256, eligible=elig)
            post = corpus.cap_topk(full, clus.to(DEV), cap, k)
            es, ei = capped_lists(z["S"], keep, clus, cap, k)
            ps, pi = post[0].cpu(), post[1].cpu()
            filled = (pi >= 0).sum(1)
            assert (filled > 0).all()
            for u in range(U):
                f = int(filled[u])
                assert torch.equal(pi[u, :f], ei[u, :f]) and torch.equal(bits(ps[u, :f]), bits(es[u, :f])), (cap, u)
                if f == k or int((full[1][u] >= 0).sum()) < 256:
                    assert torch.equal(pi[u], ei[u]), (cap, u)
            if k == 10:
                assert (filled == k).all()
            shuffled = torch.randperm(256, generator=gen).to(DEV)
            again = corpus.cap_topk((full[0][:, shuffled], full[1][:, shuffled]), clus.to(DEV), cap, k)
            assert torch.equal(again[1], post[1]) and torch.equal(bits(again[0]), bits(post[0]))
    # uncapped inputs, and a table shorter than the ids (an id at or past n_cluster is in no
    # cluster): the capped walk over exactly the news the two lists hold
    short = N // 3
    cut = clus.clone()
    cut[short:] = -1
    la = corpus.rank_topk(m, p, t, 100, news_ids=A)
    lb = corpus.rank_topk(m, p, t, 100, news_ids=B)
    held = np.zeros((U, N), bool)
    for u in range(U):
        ids = torch.cat([la[1][u], lb[1][u]]).cpu().numpy()
        held[u, ids[ids >= 0]] = True
    for table, want in ((clus, clus), (clus[:short], cut)):
        got = corpus.merge_topk(la, lb, 100, **caps_kw(table, 1))
        check_a(got, z["S"], held, want, 1, 100, ("uncapped inputs", len(table)))


def test_rank_corpus():
    """Two batch sizes give identical capped lists, equal to rank_topk on encode_users' output."""
    gen = torch.Generator().manual_seed(22)
    U, L, K, d, Dc, N = 5, 40, 32, 64, 96, 300
    table = (torch.randn(N, d, generator=gen) / d ** 0.5).to(DEV)
    mask = (torch.arange(L)[None, :] >= torch.randint(0, L - 4, (U, 1), generator=gen)).to(DEV)
    hid = torch.randint(0, N, (U, L), generator=gen).int().to(DEV)
    pk = corpus.pack_encoder((torch.randn(Dc, d, generator=gen) / d ** 0.5).to(DEV), (torch.randn(K, Dc, generator=gen) * 0.3).to(DEV),
                             (torch.randn(d, d, generator=gen) / d ** 0.5).to(DEV), dtype=torch.float32)
    clus = cluster_table(N)
    for cap in (1, 3):
        kw = caps_kw(clus, cap)
        a = corpus.rank_corpus(table, hid, mask, pk, 50, batch=2, exclude_history=True, **kw)
        b = corpus.rank_corpus(table, hid, mask, pk, 50, batch=U + 3, exclude_history=True, **kw)
        assert torch.equal(a[1], b[1]) and torch.equal(bits(a[0]), bits(b[0]))
        mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
        seen = torch.where(mask, hid, -1)
        c = corpus.rank_topk(mui, proj, table, 50, exclude_ids=seen, **kw)
        assert torch.equal(a[1], c[1]) and torch.equal(bits(a[0]), bits(c[0]))
        S = base.gpu_score_matrix(mui, proj, table, "weighted")
        check_a(a, S, base.keep_mask(U, N, seen.cpu().numpy()), clus, cap, 50, ("rank_corpus", cap))
