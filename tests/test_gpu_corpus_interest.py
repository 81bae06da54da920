"""The dominant interest of a pair and per-interest caps (miner_score_pairs_interest,
miner_rank_topk_interest, miner_topk_merge_grouped; corpus.score_pairs / rank_topk / rank_topk_deep /
rank_corpus with return_interest= / interest_cap=, merge_topk / update_topk on triples) — needs an
MI355X.

The new forms are never compared with themselves alone. Their yardsticks are
* the float64 arg-max of tests/test_interest_golden.py (table · projᵀ, respectively table · muiᵀ, from
  the operands as the device holds them) under its decisive-pair rule, and the reference's own
  interests in tests/golden/interest/corpus_interest_c5_*.npz: what an interest must be;
* A, exact: S_gpu [U, N] of the UNCAPPED ranking kernels that were there before (base.world), and
  G_gpu [U, N], the pair form's interests over the whole table (pinned by the yardstick above). The
  expected interest-capped list of user u is tests/test_gpu_corpus_cap.py's CPU walk — the lexsort of
  S_gpu[u] over the filters' survivors, the greedy cap — with G_gpu[u] as the cluster table: ids
  equal, scores bit for bit, returned interests == G_gpu. Each row must also equal, bit for bit, the
  EXISTING capped ranker on that one user with news_cluster = G_gpu[u];
* B: listed scores within tests/test_gpu_corpus_cap.py's bar of the oracle, no interest more than
  cap times, the order non-increasing with ties by id.
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_corpus_bias as biased
import test_gpu_corpus_cap as capt
import test_gpu_corpus_rankof as base
import test_interest_golden as ig
from miner_amd import _lib, corpus

# (lists that cannot fill are cases here on purpose; test_warns_when_the_list_cannot_fill checks the warning)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:rank_topk. topk=:RuntimeWarning")]
DEV = base.DEV
bits = base.bits
CASES = [c for c in base.CASES if c[1] != "mean"] + [("mid_f16", "max")]


def all_pairs(m, p, t, score_type, **kw):
    """(scores, interests) [U, N] on the CPU: the pair form over every table id."""
    U, N = m.shape[0], t.shape[0]
    ids = torch.arange(N, device=DEV).expand(U, N)
    s, g = corpus.score_pairs(m, p, t, ids, score_type=score_type, return_interest=True, **kw)
    assert s.shape == g.shape == (U, N) and g.dtype == torch.int32 and s.dtype == torch.float32
    return s.cpu(), g.cpu()


def values64(m, p, t, score_type):
    rows = p if score_type == "weighted" else m
    return ig.interest_values(t.float().cpu().numpy(), rows.float().cpu().numpy())


@functools.lru_cache(maxsize=None)
def world(shape, score_type):
    """biased.world (base.world plus the G = 3 prior) plus G_gpu and the float64 values, made once."""
    z = dict(biased.world(shape, score_type))
    z["Sp"], z["G"] = all_pairs(z["m"], z["p"], z["t"], score_type)
    z["V"] = values64(z["m"], z["p"], z["t"], score_type)
    z["K"] = z["m"].shape[1]
    return z


def check_decisive(G, V, tol, what, share=0.01):
    """G [U, N] against the float64 arg-max on every decisive pair; at most ``share`` undecided."""
    arg, _, decisive, _ = ig.dominant(V, tol)
    G = np.asarray(G)
    bad = decisive & (G != arg)
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist())
    if share is not None:
        assert ((1.0 - decisive.mean(axis=1)) <= share).all(), what


def expected_lists(S, keep, G, cap, topk):
    """Yardstick A: per user capt.capped_lists with that user's interests as the cluster table."""
    U = S.shape[0]
    rows = [capt.capped_lists(S[u:u + 1], keep[u:u + 1], G[u].numpy(), cap, topk) for u in range(U)]
    es, ei = torch.cat([r[0] for r in rows]), torch.cat([r[1] for r in rows])
    eg = torch.where(ei >= 0, torch.gather(G, 1, ei.clamp(min=0).long()), -1).int()
    return es, ei, eg


def check_a(got, S, keep, G, cap, topk, what):
    es, ei, eg = expected_lists(S, keep, G, cap, topk)
    gs, gi, gg = (x.cpu() for x in got)
    assert gs.shape == gg.shape == (S.shape[0], topk) and gi.dtype == gg.dtype == torch.int32 and gs.dtype == torch.float32
    assert torch.equal(gi, ei), (what, np.argwhere((gi != ei).numpy())[:5].tolist())
    assert torch.equal(bits(gs), bits(es)), what
    assert torch.equal(gg, eg), (what, np.argwhere((gg != eg).numpy())[:5].tolist())
    return es, ei, eg


def check_b(got, ref, tol, cap, what, prior=None):
    """Yardstick B: capt.check_b's bar (the rms over the world's oracle scores), with the returned
    interests as the groups."""
    gs, gi, gg = got[0].cpu().double().numpy(), got[1].cpu().long().numpy(), got[2].cpu().long().numpy()
    rms = float(np.sqrt(np.mean(ref ** 2)))
    add = np.zeros_like(ref) if prior is None else prior
    for u in range(gs.shape[0]):
        n = gi[u][gi[u] >= 0]
        s = gs[u][:len(n)]
        assert (gi[u][len(n):] == -1).all() and np.isneginf(gs[u][len(n):]).all() and (gg[u][len(n):] == -1).all(), what
        r = ref[u, n]
        bound = tol["rtol"] * np.abs(r) + tol["rms_floor"] * rms + capt.EPS * np.abs(s)
        assert (np.abs(s - (r + add[u, n])) <= bound).all(), what
        c = gg[u][:len(n)]
        if (c >= 0).any():
            assert np.unique(c[c >= 0], return_counts=True)[1].max() <= cap, what
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (n[:-1] < n[1:]))).all(), what


def same(a, b):
    return all(torch.equal(bits(x) if x.is_floating_point() else x, bits(y) if y.is_floating_point() else y)
               for x, y in zip(a, b)) and len(a) == len(b)


def test_the_new_surface_exists():
    for name in ("miner_score_pairs_interest", "miner_rank_topk_interest", "miner_topk_merge_grouped"):
        assert hasattr(_lib.lib(), name)


@pytest.mark.parametrize("shape,score_type", CASES)
def test_pair_interests(shape, score_type):
    """G_gpu against the float64 arg-max under the decisive-pair rule; the scores next to it are the
    old kernels' bit for bit, at C around the 256-position step with junk ids, and under the prior the
    interests are the same with biased scores; an id outside [0, N) gives -1."""
    z = world(shape, score_type)
    U, N, K, G = z["U"], z["N"], z["K"], z["G"]
    assert torch.equal(bits(z["Sp"]), bits(z["S"]))
    assert (G >= 0).all() and (G < K).all()
    check_decisive(G, z["V"], z["tol"], (shape, score_type))
    gen = torch.Generator().manual_seed(N + 5)
    for C in (1, 255, 256, 257, 600):
        cand = torch.randint(0, N, (U, C), generator=gen)
        if C > 1:
            cand[:, ::3] = -1
            cand[:, 1::5] = N
            cand[0, 0] = 2 ** 31 - 1
        valid = (cand >= 0) & (cand < N)
        want_g = torch.where(valid, torch.gather(G, 1, cand.clamp(0, N - 1)), -1).int()
        for kw in (dict(), biased.prior_kw(z)):
            plain = corpus.score_pairs(z["m"], z["p"], z["t"], cand.to(DEV), score_type=score_type, **kw)
            s, g = corpus.score_pairs(z["m"], z["p"], z["t"], cand.to(DEV), score_type=score_type, return_interest=True, **kw)
            assert torch.equal(bits(s), bits(plain)), (C, bool(kw))
            assert torch.equal(g.cpu(), want_g), (C, bool(kw))
    sb, gb = all_pairs(z["m"], z["p"], z["t"], score_type, **biased.prior_kw(z))
    assert torch.equal(gb, G) and torch.equal(bits(sb), bits(z["Sb"]))
    empty = corpus.score_pairs(z["m"], z["p"], z["t"], torch.zeros(U, 0, dtype=torch.int64, device=DEV), score_type=score_type,
                               return_interest=True)
    assert empty[0].shape == empty[1].shape == (U, 0)


TIE = (3, 19, 35)


@pytest.mark.parametrize("shape,score_type", [("mid_f16", "weighted"), ("mid_f16", "max"), ("small_f32", "weighted"),
                                              ("k20_f16", "weighted")])
def test_ties_and_the_index_mapping(shape, score_type):
    """Interest row 3 of mui and proj copied onto rows 19 and 35 where K allows — the same lane, the
    other lane half, the other interest tile — and the three scaled by 4 so that they win for most
    news: wherever the float64 arg-max is one of them (decisively against every other row), the pair
    form and the ranker must say 3. Every interest lies in [0, K)."""
    U, K, d, N, dtype = base.SHAPES[shape]
    m, p, t, _ = base.random_users(11 + K + N, U, K, d, N, dtype, dup=base.DUP)
    tie = [k for k in TIE if k < K]
    for x in (m, p):
        x[:, 3] *= 4
        for k in tie[1:]:
            x[:, k] = x[:, 3]
    V = values64(m, p, t, score_type)
    tol = base.F32_TOL if dtype == torch.float32 else base.RANK16_TOL
    arg, _, _, _ = ig.dominant(V, tol)
    assert all((V[:, :, k] == V[:, :, 3]).all() for k in tie)
    others = np.delete(V, tie[1:], axis=2)                       # the copies removed: row 3 against the rest
    _, _, decisive, _ = ig.dominant(others, tol)
    decisive &= arg == 3                                          # numpy: the lowest index of the tie
    assert decisive.mean() > 0.25, decisive.mean()
    S, G = all_pairs(m, p, t, score_type)
    G = G.numpy()
    assert (G >= 0).all() and (G < K).all()
    assert (G[decisive] == 3).all(), np.argwhere(decisive & (G != 3))[:5].tolist()
    arg_o, _, dec_o, _ = ig.dominant(others, tol)                # every other decisive pair too, in the full numbering
    full = np.array([k for k in range(K) if k not in tie[1:]])[arg_o]
    assert (G[dec_o] == full[dec_o]).all(), np.argwhere(dec_o & (G != full))[:5].tolist()
    for kw in (dict(), dict(interest_cap=7), dict(interest_cap=256)):
        s, i, g = corpus.rank_topk(m, p, t, 100, score_type=score_type, return_interest=True, **kw)
        i, g = i.cpu().long().numpy(), g.cpu().numpy()
        checked = 0
        for u in range(U):
            listed = i[u] >= 0
            assert (g[u][listed] == G[u, i[u][listed]]).all(), (kw, u)
            dec = decisive[u, i[u][listed]]
            assert (g[u][listed][dec] == 3).all(), (kw, u)
            checked += int(dec.sum())
        assert checked > 0
        if kw.get("interest_cap") == 7:
            assert all((g[u] == 3).sum() == 7 for u in range(U))


@pytest.mark.parametrize("name", ig.GOLDEN)
def test_golden_fixtures_end_to_end(name):
    """Encoded on the GPU from his_ids (fp32), the pair interests and rank_topk(return_interest=True)
    against the reference's own interests under the decisive-pair rule."""
    g = ig.load(name)
    st = g["score_type"]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    table, hid, mask = tt(g["table"]), tt(g["his_ids"]), tt(g["his_mask"])
    w2 = tt(g["W2"]) if "W2" in g else None
    pk = corpus.pack_encoder(tt(g["W1"]), tt(g["Q"]), w2, dtype=torch.float32)
    mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid, with_proj=w2 is not None)
    S, G = all_pairs(mui, proj, table, st)
    undecided = ig.check_against_golden(G.numpy(), g, ig.F32_TOL, name)
    assert (undecided[g["clicks"] >= ig.MIN_CLICKS] <= 0.02).all(), undecided
    _, _, decisive, _ = ig.dominant(ig.golden_values(g), ig.F32_TOL)
    K = int(g["K"])
    for kw in (dict(), dict(interest_cap=2)):
        s, i, gi = corpus.rank_topk(mui, proj, table, 256, score_type=st, return_interest=True, **kw)
        i, gi = i.cpu().long().numpy(), gi.cpu().numpy()
        for u in range(i.shape[0]):
            listed = i[u] >= 0
            n = i[u][listed]
            assert (gi[u][listed] == G[u].numpy()[n]).all() and (gi[u][~listed] == -1).all()
            dec = decisive[u, n]
            assert (gi[u][listed][dec] == g["interest"][u, n][dec]).all(), (name, u)
            if kw:
                assert np.bincount(gi[u][listed], minlength=K).max() <= 2


@pytest.mark.parametrize("shape,score_type", CASES)
def test_uncapped_return_interest(shape, score_type):
    """The list is the plain call's bit for bit, the interests are G_gpu at the listed ids, -1 in the
    tail (topk = 256 at N = 200: lists that end in (-inf, -1)); with filters, the subset and the prior."""
    z = world(shape, score_type)
    U, N, G = z["U"], z["N"], z["G"]
    gen = torch.Generator().manual_seed(N + 9)
    sub, _ = biased.subset_ids(gen, N)
    for kw in (dict(), dict(exclude_ids=z["hist"].to(DEV), eligible=z["ok"].to(DEV), news_ids=sub.to(DEV), **biased.prior_kw(z))):
        for topk in (10, 256):
            plain = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type, **kw)
            got = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type, return_interest=True, **kw)
            assert len(got) == 3 and same(got[:2], plain)
            i = got[1].cpu().long()
            want = torch.where(i >= 0, torch.gather(G, 1, i.clamp(min=0)), -1).int()
            assert torch.equal(got[2].cpu(), want) and got[2].dtype == torch.int32
            if topk == 256 and N < 256:
                assert (got[2][:, N:] == -1).all()


@pytest.mark.parametrize("shape,score_type", CASES)
def test_rank_topk_interest_capped(shape, score_type, monkeypatch):
    """topk 10 and 100, caps 1, 2 and 7 (cap 1 at K = 32: a list that can never fill, the threshold
    stays -inf): alone, with each filter, the 60 % subset with junk ids, the G = 3 prior, and all
    together — yardsticks A and B, and each row against the existing capped ranker with
    news_cluster = G_gpu[u]. The split switch must not change a list."""
    z = world(shape, score_type)
    U, N, G, K = z["U"], z["N"], z["G"], z["K"]
    gen = torch.Generator().manual_seed(3 * N + U)
    sub, inside = biased.subset_ids(gen, N)
    excl, ok = z["hist"], z["ok"]
    pkw = biased.prior_kw(z)
    pb = z["bias"][z["group"]].double().numpy()
    combos = [
        ("alone", dict(), z["S"], None, base.keep_mask(U, N)),
        ("excl", dict(exclude_ids=excl.to(DEV)), z["S"], None, base.keep_mask(U, N, excl.numpy())),
        ("bitmap", dict(eligible=ok.to(DEV)), z["S"], None, base.keep_mask(U, N, None, ok.numpy())),
        ("subset", dict(news_ids=sub.to(DEV)), z["S"], None, base.keep_mask(U, N) & inside[None, :]),
        ("prior", dict(**pkw), z["Sb"], pb, base.keep_mask(U, N)),
        ("all", dict(exclude_ids=excl.to(DEV), eligible=ok.to(DEV), news_ids=sub.to(DEV), **pkw), z["Sb"], pb,
         base.keep_mask(U, N, excl.numpy(), ok.numpy()) & inside[None, :]),
    ]

    def one_user(kw, u):
        """The call's keyword arguments for user u alone."""
        out = dict(kw)
        if "exclude_ids" in out:
            out["exclude_ids"] = out["exclude_ids"][u:u + 1]
        if "user_group" in out:
            out["user_group"] = out["user_group"][u:u + 1]
        return out

    for name, kw, S, prior, keep in combos:
        for topk in (10, 100):
            for cap in (1, 2, 7):
                what = (name, topk, cap)
                got = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type, interest_cap=cap,
                                       return_interest=True, **kw)
                es, ei, eg = check_a(got, S, keep, G, cap, topk, what)
                check_b(got, z["ref"], z["tol"], cap, what, prior)
                two = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type, interest_cap=cap, **kw)
                assert len(two) == 2 and same(two, got[:2]), what          # the interests are optional
                for u in range(U):                                         # every run, every row: the old capped kernel
                    old = corpus.rank_topk(z["m"][u:u + 1], None if z["p"] is None else z["p"][u:u + 1], z["t"], topk,
                                           score_type=score_type, news_cluster=G[u].to(DEV), cluster_cap=cap,
                                           **one_user(kw, u))
                    assert same(old, (got[0][u:u + 1], got[1][u:u + 1])), (what, u)
                if name == "alone" and topk == 100 and cap == 1:
                    filled = (ei >= 0).sum(1)
                    assert (filled <= K).all() and (filled < 100).all()     # K <= 64 interests: never a full list
                    plain = corpus.rank_topk(z["m"], z["p"], z["t"], topk, score_type=score_type)[1].cpu()
                    assert (plain != ei).any(dim=1).all()                   # the cap changed the answer
    name, kw, S, prior, keep = combos[-1]
    for split in ("1", "0"):
        with monkeypatch.context() as mp:
            mp.setenv("MINER_RK_SPLIT", split)
            got = corpus.rank_topk(z["m"], z["p"], z["t"], 100, score_type=score_type, interest_cap=2, return_interest=True, **kw)
            check_a(got, S, keep, G, 2, 100, ("split switch", split))


def test_warns_when_the_list_cannot_fill():
    """topk > interest_cap · K: exact (the capped test above) but slow, so the call says so; at or below
    it, and without a cap, no warning."""
    import warnings
    z = world("small_f32", "weighted")                            # K = 32
    with pytest.warns(RuntimeWarning, match="never fill"):
        corpus.rank_topk(z["m"], z["p"], z["t"], 100, interest_cap=1)
    with pytest.warns(RuntimeWarning, match="topk <= 96"):
        corpus.rank_topk(z["m"], z["p"], z["t"], 97, interest_cap=3, return_interest=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        corpus.rank_topk(z["m"], z["p"], z["t"], 32, interest_cap=1)
        corpus.rank_topk(z["m"], z["p"], z["t"], 96, interest_cap=3)
        corpus.rank_topk(z["m"], z["p"], z["t"], 100, return_interest=True)


@pytest.mark.parametrize("U", [515, 2])
def test_more_tiles_than_workgroups(U):
    """U = 515: 258 two-user tiles over at most 256 workgroups (a workgroup's second tile starts from
    empty lists and staging buffers); U = 2: one tile, where the uncapped call would take the split form."""
    K, d, N = 32, 64, 300
    m, p, t, gen = base.random_users(U + N + 2, U, K, d, N, torch.float32, dup=base.DUP)
    S = base.gpu_score_matrix(m, p, t, "weighted")
    Sp, G = all_pairs(m, p, t, "weighted")
    assert torch.equal(bits(Sp), bits(S))
    check_decisive(G, values64(m, p, t, "weighted"), base.F32_TOL, U, share=None)
    excl = torch.randint(-1, N, (U, 30), generator=gen)
    ok = torch.rand(N, generator=gen) < 0.7
    for cap in (1, 3):
        got = corpus.rank_topk(m, p, t, 100, interest_cap=cap, return_interest=True)
        check_a(got, S, base.keep_mask(U, N), G, cap, 100, ("plain", cap))
    got = corpus.rank_topk(m, p, t, 100, exclude_ids=excl.to(DEV), eligible=ok.to(DEV), interest_cap=2, return_interest=True)
    check_a(got, S, base.keep_mask(U, N, excl.numpy(), ok.numpy()), G, 2, 100, "filtered")


def test_one_chunk_per_step():
    """fp16 at d = 64: a step is one chunk, so every merge — and its read of the interests staged by
    the step before — sits between two consecutive chunk barriers."""
    U, K, d, N = 5, 32, 64, 600
    m, p, t, gen = base.random_users(66, U, K, d, N, torch.float16, dup=base.DUP)
    sub, inside = biased.subset_ids(gen, N)
    for st in ("weighted", "max"):
        S = base.gpu_score_matrix(m, p, t, st)
        Sp, G = all_pairs(m, p, t, st)
        assert torch.equal(bits(Sp), bits(S))
        check_decisive(G, values64(m, p, t, st), base.RANK16_TOL, st, share=None)
        for topk, cap in ((10, 1), (100, 2), (100, 7)):
            got = corpus.rank_topk(m, p, t, topk, score_type=st, interest_cap=cap, return_interest=True)
            check_a(got, S, base.keep_mask(U, N), G, cap, topk, (st, topk, cap))
        got = corpus.rank_topk(m, p, t, 100, score_type=st, news_ids=sub.to(DEV), interest_cap=1, return_interest=True)
        check_a(got, S, base.keep_mask(U, N) & inside[None, :], G, 1, 100, (st, "subset"))


@pytest.mark.parametrize("shape,score_type", [("small_f32", "weighted"), ("mid_f16", "weighted"), ("c5_f16", "weighted"),
                                              ("small_f32", "max")])
def test_merge_family(shape, score_type):
    """The two halves of the id range ranked with news_ids= and merged with merge_topk(interest_cap=)
    equal the interest-capped ranking of the whole table, bit for bit, interests included —
    update_topk on triples too; the grouped merge with cap 0 is merge_topk on the pairs with the
    groups carried; the b-over-a replacement takes b's group; unsorted rows work."""
    z = world(shape, score_type)
    U, N, G = z["U"], z["N"], z["G"]
    m, p, t = z["m"], z["p"], z["t"]
    gen = torch.Generator().manual_seed(N + 23)
    A, B = torch.arange(N // 2, device=DEV), torch.arange(N // 2, N, device=DEV)
    keep = base.keep_mask(U, N)
    for cap, k in ((1, 10), (2, 100), (7, 100)):
        kw = dict(score_type=score_type, interest_cap=cap, return_interest=True)
        la = corpus.rank_topk(m, p, t, k, news_ids=A, **kw)
        lb = corpus.rank_topk(m, p, t, k, news_ids=B, **kw)
        whole = corpus.rank_topk(m, p, t, k, **kw)
        check_a(whole, z["S"], keep, G, cap, k, ("whole", cap))
        merged = corpus.merge_topk(la, lb, k, interest_cap=cap)
        assert len(merged) == 3 and same(merged, whole), ("merge", cap)
        sh = torch.randperm(k, generator=gen).to(DEV)
        shuffled = corpus.merge_topk(tuple(x[:, sh] for x in la), tuple(x[:, sh] for x in lb), k, interest_cap=cap)
        assert same(shuffled, whole), ("merge unsorted", cap)
        assert same(corpus.update_topk(la, m, p, t, B, score_type=score_type, interest_cap=cap), whole), ("update", cap)
        # cap 0: the plain merge of the pairs, the groups carried
        carried = corpus.merge_topk(la, lb, k)
        plain = corpus.merge_topk(la[:2], lb[:2], k)
        assert len(carried) == 3 and same(carried[:2], plain)
        i = carried[1].cpu().long()
        assert torch.equal(carried[2].cpu(), torch.where(i >= 0, torch.gather(G, 1, i.clamp(min=0)), -1).int())
    # uncapped triples through update_topk: the uncapped ranking of the whole table with its interests
    ua = corpus.rank_topk(m, p, t, 100, score_type=score_type, news_ids=A, return_interest=True)
    assert same(corpus.update_topk(ua, m, p, t, B, score_type=score_type),
                corpus.rank_topk(m, p, t, 100, score_type=score_type, return_interest=True))
    # b over a: the same news in both lists keeps b's score and b's group
    ids = torch.arange(6, dtype=torch.int32, device=DEV).expand(U, 6).contiguous()
    a = (torch.full((U, 6), 1.0, device=DEV), ids, torch.full((U, 6), 5, dtype=torch.int32, device=DEV))
    b = (torch.full((U, 6), 0.5, device=DEV), ids, torch.full((U, 6), 9, dtype=torch.int32, device=DEV))
    out = corpus.merge_topk(a, b, 8)
    assert (out[0][:, :6] == 0.5).all() and torch.equal(out[1][:, :6], ids) and (out[2][:, :6] == 9).all()
    assert (out[1][:, 6:] == -1).all() and (out[2][:, 6:] == -1).all() and torch.isneginf(out[0][:, 6:]).all()
    out = corpus.merge_topk(a, b, 8, interest_cap=2)             # then the walk: two of group 9, the lower ids
    assert torch.equal(out[1][:, :2], ids[:, :2]) and (out[2][:, :2] == 9).all() and (out[1][:, 2:] == -1).all()
    a2 = (a[0], ids + 6, torch.tensor([-1, 5, 5, 5, -4, 9], dtype=torch.int32, device=DEV).expand(U, 6).contiguous())
    out = corpus.merge_topk(a2, b, 12, interest_cap=1)           # groups < 0 are never capped; a's 9 beats b's
    assert out[1][0].tolist()[:5] == [6, 7, 10, 11, -1] and out[2][0].tolist()[:5] == [-1, 5, -1, 9, -1]


def test_rank_corpus_and_deep_lists():
    """Two batch sizes give identical interest-capped triples, equal to rank_topk on encode_users'
    output; out= takes a triple; rank_topk_deep(return_interest=True) at topk = 300."""
    gen = torch.Generator().manual_seed(24)
    U, L, K, d, Dc, N = 5, 40, 32, 64, 96, 400
    table = (torch.randn(N, d, generator=gen) / d ** 0.5).to(DEV)
    mask = (torch.arange(L)[None, :] >= torch.randint(0, L - 4, (U, 1), generator=gen)).to(DEV)
    hid = torch.randint(0, N, (U, L), generator=gen).int().to(DEV)
    pk = corpus.pack_encoder((torch.randn(Dc, d, generator=gen) / d ** 0.5).to(DEV), (torch.randn(K, Dc, generator=gen) * 0.3).to(DEV),
                             (torch.randn(d, d, generator=gen) / d ** 0.5).to(DEV), dtype=torch.float32)
    mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
    seen = torch.where(mask, hid, -1)
    S = base.gpu_score_matrix(mui, proj, table, "weighted")
    _, G = all_pairs(mui, proj, table, "weighted")
    for cap in (1, 3):
        kw = dict(interest_cap=cap, return_interest=True)
        a = corpus.rank_corpus(table, hid, mask, pk, 50, batch=2, exclude_history=True, **kw)
        b = corpus.rank_corpus(table, hid, mask, pk, 50, batch=U + 3, exclude_history=True, **kw)
        assert len(a) == 3 and same(a, b)
        assert same(a, corpus.rank_topk(mui, proj, table, 50, exclude_ids=seen, **kw))
        check_a(a, S, base.keep_mask(U, N, seen.cpu().numpy()), G, cap, 50, ("rank_corpus", cap))
        out = (torch.empty(U, 50, device=DEV), torch.empty(U, 50, dtype=torch.int32, device=DEV),
               torch.empty(U, 50, dtype=torch.int32, device=DEV))
        assert corpus.rank_corpus(table, hid, mask, pk, 50, batch=2, exclude_history=True, out=out, **kw)[2] is out[2]
        assert same(out, a)
    c = corpus.rank_corpus(table, hid, mask, pk, 50, batch=2, return_interest=True)
    assert same(c[:2], corpus.rank_corpus(table, hid, mask, pk, 50, batch=4))
    deep = corpus.rank_topk_deep(mui, proj, table, 300, return_interest=True)
    assert len(deep) == 3 and same(deep[:2], corpus.rank_topk_deep(mui, proj, table, 300))
    i = deep[1].cpu().long()
    assert (i >= 0).all() and deep[2].shape == (U, 300)
    assert torch.equal(deep[2].cpu(), torch.gather(G, 1, i).int())
    i = c[1].cpu().long()
    assert torch.equal(c[2].cpu(), torch.gather(G, 1, i).int())
