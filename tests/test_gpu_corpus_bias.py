"""Score priors applied at rank time (miner_rank_topk_biased, miner_score_pairs_biased,
miner_rank_count_biased; the news_bias= / user_group= arguments of corpus.rank_topk, score_pairs,
rank_of, update_topk, rescore_topk, rank_corpus, evaluate_corpus) — needs an MI355X.

The biased forms are never compared with themselves alone. The yardsticks are those of
tests/test_gpu_corpus_rankof.py, with the prior added outside the library:
* A, exact: S_gpu [U, N] from the UNBIASED rank_topk (256 ids at a time), then
  Sb = S_gpu + bias[group] in torch fp32 on the CPU — one IEEE add, which is what the kernel must do.
  score_pairs(news_bias=) must equal Sb bit for bit at any ids; rank_topk(news_bias=) must return
  numpy.lexsort((ids, -Sb[u])) over the survivors of the filters, scores bit for bit and ids equal,
  unsplit and split, over the table and over news_ids, with and without exclude_ids / eligible;
  rank_of(news_bias=) must equal the lexsort rank, and a rank below 256 must sit at that position
  of the biased list.
* B, the oracle: oracle.corpus_oracle.corpus_scores plus the prior in float64, at that file's bar on
  the unbiased reference plus the rounding of the add,
  rtol·|ref| + rms_floor·rms(ref) + 2^-23·|ref + bias|; for ranks its ±2b window.
Every table repeats its rows [0, 8) at [N/2, N/2 + 8). Repeats 0-3 get equal priors (exact ties,
ranked by id); repeats 4-7 get a larger prior on the higher id, which must then rank first — the
unbiased order is the opposite one, so these tests fail without the feature. The priors are
0.5·randn, comparable to the score spread; G = 3 with user u in group u % 3, so the two users of a
workgroup tile (2t, 2t + 1) always read different rows.
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_corpus_rankof as base
from miner_amd import _lib, corpus

pytestmark = pytest.mark.gpu
DEV = base.DEV
DUP = base.DUP
G = 3
EPS = 2.0 ** -23
bits = base.bits


def make_prior(gen, N, G=G):
    """[G, N] priors, 0.5·randn; repeats 0-3 equal to their originals', repeats 4-7 larger."""
    b = 0.5 * torch.randn(G, N, generator=gen)
    h = N // 2
    b[:, h:h + 4] = b[:, :4]
    b[:, h + 4:h + DUP] = b[:, 4:DUP] + 0.25
    return b


@functools.lru_cache(maxsize=None)
def world(shape, score_type):
    """base.world plus a G = 3 prior, the groups, and both yardsticks with the prior added."""
    z = dict(base.world(shape, score_type))
    U, N = z["U"], z["N"]
    gen = torch.Generator().manual_seed(1000 + U + N)
    bias = make_prior(gen, N)
    group = torch.arange(U) % G
    z.update(bias=bias, group=group, Sb=z["S"] + bias[group], refb=z["ref"] + bias[group].double().numpy(),
             Sb1=z["S"] + bias[0][None, :], rms=float(np.sqrt(np.mean(z["ref"] ** 2))))
    return z


def prior_kw(z, g1=None):
    """The keyword arguments of a biased call: the G = 3 table with groups, or row 0 as [N] / [1, N]."""
    if g1 == "N":
        return dict(news_bias=z["bias"][0].to(DEV))
    if g1 == "1N":
        return dict(news_bias=z["bias"][:1].to(DEV))
    return dict(news_bias=z["bias"].to(DEV), user_group=z["group"].to(DEV))


def expected_lists(Sb, keep, topk):
    """numpy's order of the survivors (score desc, id asc), the first topk, then (-inf, -1)."""
    U, N = Sb.shape
    Snp = Sb.numpy()
    es = torch.full((U, topk), float("-inf"))
    ei = torch.full((U, topk), -1, dtype=torch.int32)
    for u in range(U):
        ids = np.flatnonzero(keep[u])
        order = ids[np.lexsort((ids, -Snp[u, ids].astype(np.float64)))][:topk]
        es[u, :len(order)] = Sb[u, torch.from_numpy(order)]
        ei[u, :len(order)] = torch.from_numpy(order).int()
    return es, ei


def check_lists(got, Sb, keep, topk, what):
    es, ei = expected_lists(Sb, keep, topk)
    gs, gi = got[0].cpu(), got[1].cpu()
    assert gs.shape == (Sb.shape[0], topk) and gi.dtype == torch.int32
    assert torch.equal(gi, ei), (what, np.argwhere((gi != ei).numpy())[:5].tolist())
    assert torch.equal(bits(gs), bits(es)), what


def subset_ids(gen, N):
    """About 60 % of the table in random order, with repeats and ids outside the table mixed in."""
    ids = torch.randperm(N, generator=gen)[:(6 * N) // 10]
    junk = torch.tensor([-1, N, N + 7, int(ids[0]), int(ids[1])])
    inside = np.zeros(N, bool)
    inside[ids.numpy()] = True
    return torch.cat([ids, junk]), inside


def test_the_new_surface_exists():
    for name in ("miner_rank_topk_biased", "miner_score_pairs_biased", "miner_rank_count_biased"):
        assert hasattr(_lib.lib(), name)


@pytest.mark.parametrize("shape,score_type", base.CASES)
def test_score_pairs_bits(shape, score_type):
    """Random ids with repeats, -1 and N mixed in, C around the 256-position step: yardstick A bit for
    bit (G = 3 with groups, G = 1 as [N] and as [1, N]), then the oracle's bar."""
    z = world(shape, score_type)
    U, N = z["U"], z["N"]
    gen = torch.Generator().manual_seed(N)
    tol = z["tol"]
    for C in (1, 256, 257, 600):
        cand = torch.randint(0, N, (U, C), generator=gen)
        if C > 1:
            cand[:, ::3] = -1
            cand[:, 1::5] = N
            cand[:, 2] = N // 2 + 5                               # a repeated row with a larger prior
        valid = (cand >= 0) & (cand < N)
        safe = cand.clamp(0, N - 1)
        for g1, Sb in ((None, z["Sb"]), ("N", z["Sb1"]), ("1N", z["Sb1"])):
            got = corpus.score_pairs(z["m"], z["p"], z["t"], cand.to(DEV), score_type=score_type, **prior_kw(z, g1)).cpu()
            want = torch.where(valid, torch.gather(Sb, 1, safe), float("-inf"))
            assert got.dtype == torch.float32 and torch.equal(bits(got), bits(want)), (C, g1)
        refu = np.take_along_axis(z["ref"], safe.numpy(), axis=1)
        refb = np.take_along_axis(z["refb"], safe.numpy(), axis=1)
        got = corpus.score_pairs(z["m"], z["p"], z["t"], cand.to(DEV), score_type=score_type, **prior_kw(z)).cpu()
        err = np.abs(got.double().numpy() - refb)
        bound = tol["rtol"] * np.abs(refu) + tol["rms_floor"] * z["rms"] + EPS * np.abs(refb)
        v = valid.numpy()
        print(f"{shape} {score_type} C={C}: worst err / bound {float((err[v] / bound[v]).max()):.3f}")
        assert (err[v] <= bound[v]).all(), C
    # the unbiased scores differ: the prior is not a no-op
    plain = corpus.score_pairs(z["m"], z["p"], z["t"], safe.to(DEV), score_type=score_type).cpu()
    assert not torch.equal(bits(plain), bits(got.where(valid, plain)))


@pytest.mark.parametrize("shape,score_type", base.CASES)
def test_rank_topk(shape, score_type, monkeypatch):
    """The biased lists against the lexsort of Sb: unsplit and split, table and news_ids, with and
    without the filters, a list that never fills (topk = 256 at N = 200) and one that does."""
    z = world(shape, score_type)
    U, N = z["U"], z["N"]
    gen = torch.Generator().manual_seed(3 * N)
    sub, inside = subset_ids(gen, N)
    plain = expected_lists(z["S"], base.keep_mask(U, N), 40)[1]
    for split in ("0", "1"):
        monkeypatch.setenv("MINER_RK_SPLIT", split)
        for excl, ok in ((None, None), (z["hist"], None), (None, z["ok"]), (z["hist"], z["ok"])):
            keep = base.keep_mask(U, N, None if excl is None else excl.numpy(), None if ok is None else ok.numpy())
            kw = dict(score_type=score_type, exclude_ids=None if excl is None else excl.to(DEV),
                      eligible=None if ok is None else ok.to(DEV))
            for topk in (256, 40):
                what = (split, excl is not None, ok is not None, topk)
                got = corpus.rank_topk(z["m"], z["p"], z["t"], topk, **kw, **prior_kw(z))
                check_lists(got, z["Sb"], keep, topk, what)
                if excl is None and ok is None and topk == 40:
                    gi = got[1].cpu()
                    assert all(not torch.equal(gi[u], plain[u]) for u in range(U)), "a prior that changes no list"
                got = corpus.rank_topk(z["m"], z["p"], z["t"], topk, news_ids=sub.to(DEV), **kw, **prior_kw(z))
                check_lists(got, z["Sb"], keep & inside[None, :], topk, what + ("subset",))
        for g1 in ("N", "1N"):
            got = corpus.rank_topk(z["m"], z["p"], z["t"], 40, score_type=score_type, **prior_kw(z, g1))
            check_lists(got, z["Sb1"], base.keep_mask(U, N), 40, (split, g1))
    # the repeated rows, through the list: copies 0-3 adjacent with the lower id first, 4-7 the higher id first
    monkeypatch.setenv("MINER_RK_SPLIT", "0")
    ids = torch.cat([torch.arange(DUP), N // 2 + torch.arange(DUP)])
    gi = corpus.rank_topk(z["m"], z["p"], z["t"], 2 * DUP, score_type=score_type, news_ids=ids.to(DEV), **prior_kw(z))[1].cpu()
    pi = corpus.rank_topk(z["m"], z["p"], z["t"], 2 * DUP, score_type=score_type, news_ids=ids.to(DEV))[1].cpu()
    for u in range(U):
        pos = {int(n): k for k, n in enumerate(gi[u])}
        ppos = {int(n): k for k, n in enumerate(pi[u])}
        for i in range(DUP):
            assert ppos[N // 2 + i] == ppos[i] + 1                # unbiased: always the lower id first
            if i < 4:
                assert pos[N // 2 + i] == pos[i] + 1, (u, i)
            else:
                assert pos[N // 2 + i] < pos[i], (u, i)


def check_rank_of(z, score_type, tid, excl, ok, Sb, refb, kw):
    """rank_of under a prior and the filters against yardsticks A and B."""
    U, N, tol = z["U"], z["N"], z["tol"]
    fkw = dict(score_type=score_type, exclude_ids=None if excl is None else excl.to(DEV),
               eligible=None if ok is None else ok.to(DEV))
    ranks, scores = corpus.rank_of(z["m"], z["p"], z["t"], tid.to(DEV), **fkw, **kw)
    assert ranks.dtype == torch.int32 and scores.dtype == torch.float32 and ranks.shape == scores.shape == tid.shape
    ranks, scores = ranks.cpu().numpy().astype(np.int64), scores.cpu()
    keep = base.keep_mask(U, N, None if excl is None else excl.numpy(), None if ok is None else ok.numpy())
    keep &= ~np.isnan(Sb.numpy())                                  # a NaN score is in no list
    tnp = tid.long().numpy()
    want = base.lexsort_ranks(Sb.numpy(), keep, tnp)
    assert np.array_equal(ranks, want), f"ranks differ from the lexsort at {np.argwhere(ranks != want)[:5].tolist()}"
    valid = (tid >= 0) & (tid < N)
    want_s = torch.where(valid, torch.gather(Sb, 1, tid.long().clamp(0, N - 1)), float("-inf"))
    same = bits(scores) == bits(want_s)
    assert bool((same | (torch.isnan(scores) & torch.isnan(want_s))).all())
    listed = corpus.rank_topk(z["m"], z["p"], z["t"], 256, **fkw, **kw)[1].cpu().numpy()
    for u, j in zip(*np.nonzero((ranks >= 0) & (ranks < 256))):
        assert listed[u, ranks[u, j]] == tnp[u, j], (u, j)
    if refb is not None:                                          # the oracle's window
        for u, j in zip(*np.nonzero(ranks >= 0)):
            s, n = float(scores[u, j]), tnp[u, j]
            b = tol["rtol"] * abs(z["ref"][u, n]) + tol["rms_floor"] * z["rms"] + EPS * abs(refb[u, n])
            alive = refb[u][keep[u]]
            assert (alive > s + 2 * b).sum() <= ranks[u, j] <= (alive >= s - 2 * b).sum(), (u, j)
    return ranks


@pytest.mark.parametrize("shape,score_type", base.CASES)
def test_rank_of(shape, score_type):
    """T = 1 and 64, without filters and with the bitmap and padded histories; G = 3 and G = 1."""
    z = world(shape, score_type)
    U, N = z["U"], z["N"]
    gen = torch.Generator().manual_seed(U + N)
    for T in (1, 64):
        tid = base.targets_for(z, T, gen)
        hist = z["hist"].clone()
        hist[0, 10] = tid[0, 0]
        for excl, ok in ((None, None), (None, z["ok"]), (hist, z["ok"])):
            ranks = check_rank_of(z, score_type, tid, excl, ok, z["Sb"], z["refb"], prior_kw(z))
            if T == 64 and excl is None and ok is None:
                assert (ranks[:, 4:6] == -1).all()                         # ids -1 and N
                lo, hi = ranks[:, 5 + np.arange(1, DUP)], ranks[:, 13 + np.arange(1, DUP)]   # ids i and N/2 + i
                assert (hi[:, :3] == lo[:, :3] + 1).all()                  # equal priors: the lower id first, adjacent
                assert (hi[:, 3:] < lo[:, 3:]).all()                       # a larger prior on the higher id: it ranks first
            if excl is not None:
                assert ranks[0, 0] == -1                                   # in its own exclusion list
    check_rank_of(z, score_type, base.targets_for(z, 64, gen), None, None, z["Sb1"], None, prior_kw(z, "N"))
    check_rank_of(z, score_type, base.targets_for(z, 64, gen), None, z["ok"], z["Sb1"], None, prior_kw(z, "1N"))


@pytest.mark.parametrize("shape", ["small_f32", "mid_f16"])
def test_nonfinite_priors(shape, monkeypatch):
    """A +inf, a -inf and a NaN prior on three news, no special case anywhere: +inf ranks first, -inf is
    listed only while the list is not full, the NaN sum is in no list and gets rank -1."""
    z = world(shape, "weighted")
    U, N = z["U"], z["N"]
    a, b, c = 17, N // 2 + 2, N - 3
    bias = z["bias"][0].clone()
    bias[a], bias[b], bias[c] = float("inf"), float("-inf"), float("nan")
    Sb = z["S"] + bias[None, :]
    keep = base.keep_mask(U, N)
    keep[:, c] = False                                            # masked out of the yardstick's survivors
    kw = dict(news_bias=bias.to(DEV))
    for split in ("0", "1"):
        monkeypatch.setenv("MINER_RK_SPLIT", split)
        for topk in (256, 40):
            got = corpus.rank_topk(z["m"], z["p"], z["t"], topk, **kw)
            check_lists(got, Sb, keep, topk, (split, topk))
            gi = got[1].cpu()
            assert (gi[:, 0] == a).all() and not (gi == c).any()
            assert (gi == b).any() == (topk >= N - 1)             # N = 200: the list has room; otherwise it is full
    tid = torch.tensor([[a, b, c, 0]]).expand(U, 4).contiguous()
    ranks = check_rank_of(z, "weighted", tid, None, None, Sb, None, kw)
    assert (ranks[:, 0] == 0).all() and (ranks[:, 1] == N - 2).all() and (ranks[:, 2] == -1).all()
    got = corpus.score_pairs(z["m"], z["p"], z["t"], tid.to(DEV), **kw).cpu()
    assert torch.isnan(got[:, 2]).all() and torch.equal(bits(got[:, [0, 1, 3]]), bits(Sb[:, [a, b, 0]]))


@pytest.mark.parametrize("U", [515, 2])
def test_more_tiles_than_workgroups(U):
    """U = 515: 258 two-user tiles with an odd last one (ranking and counting forms) and 515 one-user
    tiles (pair form) over at most 256 workgroups: the prior row changes with the tile while the issue
    side is already in the next one. U = 2: one tile, two groups."""
    K, d, N = 32, 64, 300
    m, p, t, gen = base.random_users(U + N, U, K, d, N, torch.float32, dup=DUP)
    S = base.gpu_score_matrix(m, p, t, "weighted")
    bias = make_prior(gen, N)
    group = torch.arange(U) % G
    Sb = S + bias[group]
    kw = dict(news_bias=bias.to(DEV), user_group=group.to(DEV))
    cand = torch.randint(-1, N + 1, (U, 300), generator=gen)
    got = corpus.score_pairs(m, p, t, cand.to(DEV), **kw).cpu()
    valid = (cand >= 0) & (cand < N)
    assert torch.equal(bits(got), bits(torch.where(valid, torch.gather(Sb, 1, cand.clamp(0, N - 1)), float("-inf"))))
    tid = torch.randint(0, N, (U, 3), generator=gen)
    tid[:, 2] = N // 2 + torch.arange(U) % DUP
    excl = torch.randint(-1, N, (U, 30), generator=gen)
    ok = torch.rand(N, generator=gen) < 0.7
    fkw = dict(exclude_ids=excl.to(DEV), eligible=ok.to(DEV))
    keep = base.keep_mask(U, N, excl.numpy(), ok.numpy())
    ranks, scores = corpus.rank_of(m, p, t, tid.to(DEV), **fkw, **kw)
    assert np.array_equal(ranks.cpu().numpy().astype(np.int64), base.lexsort_ranks(Sb.numpy(), keep, tid.numpy()))
    assert torch.equal(bits(scores.cpu()), bits(torch.gather(Sb, 1, tid)))
    sub, inside = subset_ids(gen, N)
    check_lists(corpus.rank_topk(m, p, t, 100, **fkw, **kw), Sb, keep, 100, "table")
    check_lists(corpus.rank_topk(m, p, t, 100, news_ids=sub.to(DEV), **fkw, **kw), Sb, keep & inside[None, :], 100, "subset")
    # int64 groups, and an int8 tensor, are the same groups
    check_lists(corpus.rank_topk(m, p, t, 20, news_bias=bias.to(DEV), user_group=group.to(DEV, torch.int8)), Sb,
                base.keep_mask(U, N), 20, "int8 groups")


def test_one_chunk_per_step():
    """fp16 at d = 64: a news row is one 128-byte chunk, a step one chunk — the step's priors (and, in
    the gathering forms, the ids they are read at) are loaded and used within the same chunk."""
    U, K, d, N = 5, 32, 64, 600
    m, p, t, gen = base.random_users(64, U, K, d, N, torch.float16, dup=DUP)
    bias = make_prior(gen, N)
    group = torch.arange(U) % G
    kw = dict(news_bias=bias.to(DEV), user_group=group.to(DEV))
    sub, inside = subset_ids(gen, N)
    for st in ("weighted", "mean"):
        Sb = base.gpu_score_matrix(m, p, t, st) + bias[group]
        cand = torch.randint(0, N, (U, 300), generator=gen)
        got = corpus.score_pairs(m, p, t, cand.to(DEV), score_type=st, **kw).cpu()
        assert torch.equal(bits(got), bits(torch.gather(Sb, 1, cand))), st
        tid = torch.cat([torch.randint(0, N, (U, 5), generator=gen), torch.tensor([[0, N // 2, N // 2 + 6, N - 1]]).expand(U, 4)], dim=1)
        ranks, _ = corpus.rank_of(m, p, t, tid.to(DEV), score_type=st, **kw)
        assert np.array_equal(ranks.cpu().numpy().astype(np.int64), base.lexsort_ranks(Sb.numpy(), base.keep_mask(U, N), tid.numpy())), st
        check_lists(corpus.rank_topk(m, p, t, 100, score_type=st, **kw), Sb, base.keep_mask(U, N), 100, st)
        check_lists(corpus.rank_topk(m, p, t, 100, score_type=st, news_ids=sub.to(DEV), **kw), Sb,
                    base.keep_mask(U, N) & inside[None, :], 100, (st, "subset"))


def test_update_and_rescore_under_a_prior():
    """update_topk(rank(A), B) under a prior is rank(A ∪ B) under it; rescore_topk(news_bias=) is, row by
    row, rank_topk(news_ids=<the old ids>, news_bias=)."""
    z = world("mid_f16", "weighted")
    U, N, k = z["U"], z["N"], 100
    kw = prior_kw(z)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    A, B = perm[:N // 2].to(DEV), perm[N // 2:(3 * N) // 4].to(DEV)
    ok = z["ok"].to(DEV)
    for elig in (None, ok):
        first = corpus.rank_topk(z["m"], z["p"], z["t"], k, news_ids=A, eligible=elig, **kw)
        got = corpus.update_topk(first, z["m"], z["p"], z["t"], B, eligible=elig, **kw)
        want = corpus.rank_topk(z["m"], z["p"], z["t"], k, news_ids=torch.cat([A, B]), eligible=elig, **kw)
        assert torch.equal(got[1], want[1]) and torch.equal(bits(got[0]), bits(want[0]))
        inside = np.zeros(N, bool)
        inside[torch.cat([A, B]).cpu().numpy()] = True
        keep = base.keep_mask(U, N, None, None if elig is None else z["ok"].numpy()) & inside[None, :]
        check_lists(got, z["Sb"], keep, k, "update")
    old = corpus.rank_topk(z["m"], z["p"], z["t"], k)             # served lists ranked without a prior
    for elig in (None, ok):
        got = corpus.rescore_topk(old, z["m"], z["p"], z["t"], eligible=elig, **kw)
        for u in range(U):
            ids = old[1][u][old[1][u] >= 0]
            want = corpus.rank_topk(z["m"][u:u + 1], z["p"][u:u + 1], z["t"], k, news_ids=ids, eligible=elig,
                                    news_bias=kw["news_bias"], user_group=kw["user_group"][u:u + 1])
            assert torch.equal(bits(got[0][u:u + 1]), bits(want[0])) and torch.equal(got[1][u:u + 1], want[1]), u
    assert not torch.equal(got[1], old[1])


def test_rank_corpus_and_evaluate_corpus():
    """Two batch sizes give identical lists and ranks under a prior (user_group sliced per batch), equal
    to rank_topk / rank_of on encode_users' output."""
    gen = torch.Generator().manual_seed(21)
    U, L, K, d, Dc, N, T = 5, 40, 32, 64, 96, 200, 4
    table = (torch.randn(N, d, generator=gen) / d ** 0.5).to(DEV)
    mask = (torch.arange(L)[None, :] >= torch.randint(0, L - 4, (U, 1), generator=gen)).to(DEV)
    hid = torch.randint(0, N, (U, L), generator=gen).int().to(DEV)
    pk = corpus.pack_encoder((torch.randn(Dc, d, generator=gen) / d ** 0.5).to(DEV), (torch.randn(K, Dc, generator=gen) * 0.3).to(DEV),
                             (torch.randn(d, d, generator=gen) / d ** 0.5).to(DEV), dtype=torch.float32)
    tid = torch.randint(0, N, (U, T), generator=gen).to(DEV)
    kw = dict(news_bias=make_prior(gen, N).to(DEV), user_group=(torch.arange(U) % G).to(DEV))
    mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
    seen = torch.where(mask, hid, -1)
    a = corpus.rank_corpus(table, hid, mask, pk, 50, batch=2, exclude_history=True, **kw)
    b = corpus.rank_corpus(table, hid, mask, pk, 50, batch=U + 3, exclude_history=True, **kw)
    c = corpus.rank_topk(mui, proj, table, 50, exclude_ids=seen, **kw)
    for x in (b, c):
        assert torch.equal(a[1], x[1]) and torch.equal(bits(a[0]), bits(x[0]))
    assert not torch.equal(a[1], corpus.rank_corpus(table, hid, mask, pk, 50, exclude_history=True)[1])
    ra, ma = corpus.evaluate_corpus(table, hid, mask, pk, tid, batch=2, **kw)
    rb, mb = corpus.evaluate_corpus(table, hid, mask, pk, tid, batch=U + 3, **kw)
    rc, _ = corpus.rank_of(mui, proj, table, tid, exclude_ids=seen, **kw)
    assert torch.equal(ra, rb) and torch.equal(ra, rc)
    assert all(ma[k] == mb[k] or (np.isnan(ma[k]) and np.isnan(mb[k])) for k in ma)
    listed = corpus.rank_topk(mui, proj, table, 256, exclude_ids=seen, **kw)[1]
    for u, j in zip(*np.nonzero(ra.cpu().numpy() >= 0)):
        assert listed[u, ra[u, j]].item() == tid[u, j].item()


@pytest.mark.parametrize("shape", ["small_f32", "c5_f16"])
def test_zero_and_absent_priors(shape, monkeypatch):
    """news_bias = zeros: the unbiased ids, and scores equal as floats (adding +0 may turn -0 into
    +0). news_bias = None, and a NULL table at the C entry points: today's result bit for bit."""
    z = world(shape, "weighted")
    U, K, d, N, dtype = base.SHAPES[shape]
    m, p, t = z["m"], z["p"], z["t"]
    zero = torch.zeros(N, device=DEV)
    cand = torch.randint(-1, N + 1, (U, 70), generator=torch.Generator().manual_seed(9)).to(DEV)
    sub = torch.arange(0, N, 3, device=DEV)
    for split in ("0", "1"):
        monkeypatch.setenv("MINER_RK_SPLIT", split)
        for kw in (dict(), dict(news_ids=sub), dict(eligible=z["ok"].to(DEV), exclude_ids=z["hist"].to(DEV))):
            want = corpus.rank_topk(m, p, t, 100, **kw)
            got = corpus.rank_topk(m, p, t, 100, news_bias=zero, **kw)
            assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
            none = corpus.rank_topk(m, p, t, 100, news_bias=None, user_group=None, **kw)
            assert torch.equal(none[1], want[1]) and torch.equal(bits(none[0]), bits(want[0]))
    want = corpus.score_pairs(m, p, t, cand)
    assert torch.equal(corpus.score_pairs(m, p, t, cand, news_bias=zero), want)
    assert torch.equal(bits(corpus.score_pairs(m, p, t, cand, news_bias=None)), bits(want))
    tid = cand[:, :9]
    want = corpus.rank_of(m, p, t, tid, eligible=z["ok"].to(DEV))
    got = corpus.rank_of(m, p, t, tid, eligible=z["ok"].to(DEV), news_bias=zero)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the C entry points with a NULL table forward to the unbiased instantiations
    lib = _lib.lib()
    dt, st = corpus._DT[dtype], _lib.SCORE_WEIGHTED
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda x: None if x is None else x.data_ptr()
    sub32 = sub.int()
    for ids, M in ((None, -1), (sub32, sub32.numel())):
        want = corpus.rank_topk(m, p, t, 100, news_ids=None if ids is None else sub)
        s = torch.empty(U, 100, dtype=torch.float32, device=DEV)
        i = torch.empty(U, 100, dtype=torch.int32, device=DEV)
        rc = lib.miner_rank_topk_biased(stream, dt, st, ptr(m), ptr(p), ptr(t), U, N, d, K, 100, None, 0, None, ptr(ids), M,
                                        ptr(s), ptr(i), None, 0, None, 0, None)
        assert rc == 0 and torch.equal(i, want[1]) and torch.equal(bits(s), bits(want[0]))
    c32 = cand.int().contiguous()
    out = torch.empty(U, 70, dtype=torch.float32, device=DEV)
    rc = lib.miner_score_pairs_biased(stream, dt, st, ptr(m), ptr(p), ptr(t), U, N, d, K, ptr(c32), 70, ptr(out), None, 0, None)
    assert rc == 0 and torch.equal(bits(out), bits(corpus.score_pairs(m, p, t, cand)))
