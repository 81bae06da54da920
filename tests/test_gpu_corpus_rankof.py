"""Scores of given pairs and exact full-corpus ranks (miner_score_pairs, miner_rank_count;
corpus.score_pairs / rank_of / evaluate_corpus / rescore_topk) — needs an MI355X.

The new forms are never compared with themselves alone. Their yardsticks are
* A, exact: the full score matrix S_gpu [U, N] of the ranking kernels that were there before
  (rank_topk(topk=256, news_ids=<256 ids at a time>), scattered by the returned ids). score_pairs
  must equal it bit for bit at any ids, rank_of must equal the rank numpy's lexsort((ids, -S_gpu[u]))
  gives under the filters (keep_mask), and a target ranked below 256 must sit at that position of
  rank_topk's list under the same filters;
* B, the oracle (oracle.corpus_oracle.corpus_scores) at the bars of tests/test_gpu_corpus_filter.py:
  fp32 1e-5·|ref| + 1e-5·rms, 16-bit 2e-4 / 2e-4. With b that bound at the target's score s,
  #{ref > s + 2b} <= rank <= #{ref >= s - 2b} over the survivors.
Every table repeats its rows [0, 8) at [N/2, N/2 + 8): exact ties, ordered by id, and a target
that must not count itself.
"""
import functools

import numpy as np
import pytest
import torch

from miner_amd import corpus
from oracle import corpus_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_TOL = dict(rtol=1e-5, rms_floor=1e-5)          # the bars of tests/test_gpu_corpus_filter.py
RANK16_TOL = dict(rtol=2e-4, rms_floor=2e-4)
DUP = 8

# name -> (U, K, d, N, dtype): the smallest shapes at which each mechanism can break
SHAPES = {
    "small_f32": (5, 32, 64, 200, torch.float32),      # one partial step; odd U: a tile with a user past U
    "mid_f16": (3, 64, 128, 1000, torch.float16),      # three full 256-steps + 232 rows; two interest tiles
    "mid_f32": (3, 64, 128, 1000, torch.float32),
    "c5_f16": (3, 64, 768, 600, torch.float16),        # K and the chunk count compile-time (config 5)
    "c5_bf16": (3, 64, 768, 600, torch.bfloat16),
    "k20_f16": (4, 20, 768, 300, torch.float16),       # d = 768 with K at run time
}
CASES = [("small_f32", "weighted"), ("small_f32", "max"), ("small_f32", "mean"), ("mid_f16", "weighted"),
         ("mid_f32", "weighted"), ("c5_f16", "weighted"), ("c5_bf16", "weighted"), ("k20_f16", "weighted")]


def keep_mask(U, N, excl=None, ok=None):
    """bool [U,N]: the (user, news) pairs the filters let through (tests/test_gpu_corpus_filter.py)."""
    keep = np.ones((U, N), bool)
    if ok is not None:
        keep &= np.asarray(ok, bool)[None, :]
    if excl is not None:
        excl = np.asarray(excl, np.int64)
        for u in range(U):
            ids = excl[u][(excl[u] >= 0) & (excl[u] < N)]
            keep[u, ids] = False
    return keep


def random_users(seed, U, K, d, N, dtype, dup=0):
    """Random user vectors and a table; the table's rows [N/2, N/2 + dup) repeat rows [0, dup)."""
    gen = torch.Generator().manual_seed(seed)
    mui = torch.randn(U, K, d, generator=gen) / 2
    proj = torch.randn(U, K, d, generator=gen) / 2
    table = torch.randn(N, d, generator=gen) / d ** 0.5
    if dup:
        table[N // 2:N // 2 + dup] = table[:dup]
    m, p, t = (x.to(DEV, dtype) for x in (mui, proj, table))
    return m, p, t, gen


def gpu_score_matrix(m, p, t, score_type):
    """S_gpu [U, N] fp32 (CPU) from rank_topk alone: 256 ids at a time, every one of them returned."""
    U, N = m.shape[0], t.shape[0]
    S = torch.full((U, N), float("nan"))
    for lo in range(0, N, 256):
        ids = torch.arange(lo, min(N, lo + 256), device=DEV)
        ts, ti = corpus.rank_topk(m, p, t, 256, score_type=score_type, news_ids=ids)
        ts, ti = ts.cpu(), ti.cpu().long()
        assert ((ti >= 0).sum(1) == len(ids)).all()
        for u in range(U):
            S[u, ti[u, :len(ids)]] = ts[u, :len(ids)]
    assert not torch.isnan(S).any()
    return S


@functools.lru_cache(maxsize=None)
def world(shape, score_type):
    """Users, table, S_gpu, the oracle's scores and the bar of one (shape, score type), made once."""
    U, K, d, N, dtype = SHAPES[shape]
    m, p, t, gen = random_users(7 + len(shape) + K + N, U, K, d, N, dtype, dup=DUP)
    S = gpu_score_matrix(m, p, t, score_type)
    ref = co.corpus_scores(m.float().cpu(), p.float().cpu(), t.float().cpu(), score_type).double().numpy()
    hist = torch.randint(0, N, (U, 40), generator=gen)          # padded histories with repeats
    hist[:, :7] = -1
    hist[:, 8] = hist[:, 9]
    ok = torch.rand(N, generator=gen) < 0.6
    ok[N - 1] = False                                            # news N - 1 is a target below: ineligible
    return dict(U=U, N=N, m=m, p=p, t=t, S=S, Snp=S.numpy(), ref=ref, hist=hist, ok=ok,
                tol=F32_TOL if dtype == torch.float32 else RANK16_TOL)


def bits(x):
    return x.contiguous().view(torch.int32)


def lexsort_ranks(S, keep, tid):
    """Rank of every target in numpy's order of the survivors (score desc, id asc); -1 outside it."""
    U, N = S.shape
    out = np.full(tid.shape, -1, np.int64)
    for u in range(U):
        ids = np.flatnonzero(keep[u])
        order = ids[np.lexsort((ids, -S[u, ids].astype(np.float64)))]
        pos = np.full(N, -1, np.int64)
        pos[order] = np.arange(len(order))
        for j, n in enumerate(tid[u]):
            if 0 <= n < N:
                out[u, j] = pos[n]
    return out


def targets_for(z, T, gen):
    """[U, T] targets: T = 1 each user's best news; T = 3 its worst, news N - 1, news 0; T = 64 all of
    those, both copies of every repeated row, an id on either side of the table, random others."""
    U, N, S = z["U"], z["N"], z["Snp"]
    order = [np.lexsort((np.arange(N), -S[u].astype(np.float64))) for u in range(U)]
    best = torch.tensor([int(o[0]) for o in order])[:, None]
    worst = torch.tensor([int(o[-1]) for o in order])[:, None]
    col = lambda v: torch.full((U, 1), v)
    if T == 1:
        return best
    if T == 3:
        return torch.cat([worst, col(N - 1), col(0)], dim=1)
    fixed = [best, worst, col(N - 1), col(0), col(-1), col(N)]
    fixed += [col(n) for n in range(1, DUP)] + [col(N // 2 + n) for n in range(DUP)]
    fixed = torch.cat(fixed, dim=1)
    rest = torch.randint(0, N, (U, T - fixed.shape[1]), generator=gen)
    return torch.cat([fixed, rest], dim=1)


def test_the_new_surface_exists():
    for name in ("score_pairs", "rank_of", "corpus_metrics", "evaluate_corpus", "rescore_topk"):
        assert callable(getattr(corpus, name)), name


@pytest.mark.parametrize("shape,score_type", CASES)
def test_score_pairs_bits(shape, score_type):
    """C around the 256-position step; random ids with repeats, in descending order, with -1 and N
    mixed in; int32 and int64. Yardstick A bit for bit, then the oracle's bar."""
    z = world(shape, score_type)
    U, N, S = z["U"], z["N"], z["S"]
    gen = torch.Generator().manual_seed(N)
    rms = float(np.sqrt(np.mean(z["ref"] ** 2)))
    for C in (1, 255, 256, 257, 600):
        ids = torch.randint(0, N, (U, C), generator=gen)         # repeats whenever C > N, and mostly before
        lists = {"random": ids, "descending": torch.sort(ids, dim=1, descending=True).values}
        junk = ids.clone()
        junk[:, ::3] = -1
        junk[:, 1::5] = N
        junk[0, 0] = 2 ** 31 - 1
        lists["junk"] = junk
        if C == 1:
            lists["last"] = torch.full((U, 1), N - 1)
            lists["first"] = torch.zeros(U, 1, dtype=torch.int64)
        for name, cand in lists.items():
            for dt in ((torch.int64, torch.int32) if name == "junk" else (torch.int64,)):
                got = corpus.score_pairs(z["m"], z["p"], z["t"], cand.to(DEV, dt), score_type=score_type).cpu()
                assert got.shape == (U, C) and got.dtype == torch.float32
                valid = (cand >= 0) & (cand < N)
                want = torch.where(valid, torch.gather(S, 1, cand.clamp(0, N - 1)), float("-inf"))
                assert torch.equal(bits(got), bits(want)), (C, name)
                refs = np.take_along_axis(z["ref"], cand.clamp(0, N - 1).numpy(), axis=1)
                err = np.abs(got.double().numpy() - refs)[valid.numpy()]
                bound = (z["tol"]["rtol"] * np.abs(refs) + z["tol"]["rms_floor"] * rms)[valid.numpy()]
                assert (err <= bound).all(), (C, name)
    empty = corpus.score_pairs(z["m"], z["p"], z["t"], torch.zeros(U, 0, dtype=torch.int64, device=DEV), score_type=score_type)
    assert empty.shape == (U, 0)


def check_rank_of(z, score_type, tid, excl, ok, packed=False, listed=None):
    """rank_of under the filters against yardsticks A and B (see the module docstring)."""
    U, N, S, ref, tol = z["U"], z["N"], z["Snp"], z["ref"], z["tol"]
    elig = None if ok is None else (corpus.pack_eligible(ok.to(DEV)) if packed else ok.to(DEV))
    ranks, scores = corpus.rank_of(z["m"], z["p"], z["t"], tid.to(DEV), score_type=score_type,
                                   exclude_ids=None if excl is None else excl.to(DEV), eligible=elig)
    assert ranks.dtype == torch.int32 and scores.dtype == torch.float32 and ranks.shape == scores.shape == tid.shape
    ranks, scores = ranks.cpu().numpy().astype(np.int64), scores.cpu()
    keep = keep_mask(U, N, None if excl is None else excl.numpy(), None if ok is None else ok.numpy())
    t64 = tid.long()
    tnp = t64.numpy()
    want = lexsort_ranks(S, keep, tnp)
    assert np.array_equal(ranks, want), f"ranks differ from the lexsort at {np.argwhere(ranks != want)[:5].tolist()}"
    valid = (t64 >= 0) & (t64 < N)
    want_s = torch.where(valid, torch.gather(z["S"], 1, t64.clamp(0, N - 1)), float("-inf"))
    assert torch.equal(bits(scores), bits(want_s))
    # the position in the list rank_topk serves under the same filters
    if listed is not None:
        for u, j in zip(*np.nonzero((ranks >= 0) & (ranks < 256))):
            assert listed[u, ranks[u, j]] == tnp[u, j], (u, j)
    # the oracle's window
    rms = float(np.sqrt(np.mean(ref ** 2)))
    for u, j in zip(*np.nonzero(ranks >= 0)):
        s = float(scores[u, j])
        b = tol["rtol"] * abs(s) + tol["rms_floor"] * rms
        alive = ref[u][keep[u]]
        assert (alive > s + 2 * b).sum() <= ranks[u, j] <= (alive >= s - 2 * b).sum(), (u, j)
    return ranks


@pytest.mark.parametrize("shape,score_type", CASES)
def test_rank_of(shape, score_type):
    """T = 1, 3, 64 without filters, with the bitmap (bool and packed; news N - 1 ineligible), with
    padded histories as exclude_ids (user 0's first target in its own list), and with both."""
    z = world(shape, score_type)
    U, N = z["U"], z["N"]
    gen = torch.Generator().manual_seed(U + N)
    for T in (1, 3, 64):
        tid = targets_for(z, T, gen)
        hist = z["hist"].clone()
        hist[0, 10] = tid[0, 0]
        for name, excl, ok, packed in (("none", None, None, False), ("bitmap", None, z["ok"], False),
                                       ("packed", None, z["ok"], True), ("history", hist, None, False),
                                       ("both", hist, z["ok"], True)):
            elig = None if ok is None else ok.to(DEV)
            listed = corpus.rank_topk(z["m"], z["p"], z["t"], 256, score_type=score_type, eligible=elig,
                                      exclude_ids=None if excl is None else excl.to(DEV))[1].cpu().numpy()
            ranks = check_rank_of(z, score_type, tid, excl, ok, packed, listed)
            survivors = keep_mask(U, N, None if excl is None else excl.numpy(), None if ok is None else ok.numpy()).sum(1)
            if name == "none":
                if T == 1:
                    assert (ranks == 0).all()                              # each user's best news
                if T == 3:
                    assert (ranks[:, 0] == N - 1).all()                    # its worst: rank = survivors - 1
                if T == 64:
                    assert (ranks[:, 4:6] == -1).all()                     # ids -1 and N
                    lo, hi = ranks[:, 6 + np.arange(DUP - 1)], ranks[:, 6 + DUP + np.arange(DUP - 1)]
                    assert (hi == lo + 1).all()                            # a repeated row: the lower id first, adjacent
            if excl is not None:
                assert ranks[0, 0] == -1                                   # in its own exclusion list
            if ok is not None and T >= 3:
                assert (ranks[:, 1 if T == 3 else 2] == -1).all()          # news N - 1: not eligible
            if T == 3 and name != "none":
                w = ranks[:, 0]
                assert ((w == -1) | (w == survivors - 1)).all()            # the worst news: last, or filtered
    # (the worst of all N news is the worst of the survivors whenever it survives)


def test_exclusion_widths():
    """exclude_ids of width 0 (no exclusion) and of width 256, the cap: random ids, -1 slots, repeats."""
    z = world("small_f32", "weighted")
    U, N = z["U"], z["N"]
    gen = torch.Generator().manual_seed(256)
    tid = targets_for(z, 64, gen)
    a = check_rank_of(z, "weighted", tid, torch.zeros(U, 0, dtype=torch.int64), None)
    b = check_rank_of(z, "weighted", tid, None, None)
    assert np.array_equal(a, b)
    wide = torch.randint(-1, N, (U, 256), generator=gen)
    wide[:, ::4] = -1
    assert len(set(wide[0].tolist())) < 256 - 64                 # repeats
    check_rank_of(z, "weighted", tid, wide, z["ok"])
    check_rank_of(z, "weighted", tid.to(torch.int32), wide.to(torch.int32), z["ok"])


@pytest.mark.parametrize("U", [515, 2])
def test_more_tiles_than_workgroups(U):
    """U = 515: 258 two-user tiles (counting form) and 515 one-user tiles (pair form) over at most 256
    workgroups — the issue side's rows and ids cross tile boundaries while another tile is being
    computed; every user has its own candidate list, exclusion list and targets. U = 2: one tile."""
    K, d, N = 32, 64, 300
    m, p, t, gen = random_users(U + N, U, K, d, N, torch.float32, dup=DUP)
    S = gpu_score_matrix(m, p, t, "weighted")
    cand = torch.randint(-1, N + 1, (U, 300), generator=gen)
    got = corpus.score_pairs(m, p, t, cand.to(DEV)).cpu()
    valid = (cand >= 0) & (cand < N)
    want = torch.where(valid, torch.gather(S, 1, cand.clamp(0, N - 1)), float("-inf"))
    assert torch.equal(bits(got), bits(want))
    tid = torch.randint(0, N, (U, 3), generator=gen)
    tid[:, 2] = N // 2 + torch.arange(U) % DUP                   # a repeated row's second copy
    excl = torch.randint(-1, N, (U, 30), generator=gen)
    ok = torch.rand(N, generator=gen) < 0.7
    ranks, scores = corpus.rank_of(m, p, t, tid.to(DEV), exclude_ids=excl.to(DEV), eligible=ok.to(DEV))
    keep = keep_mask(U, N, excl.numpy(), ok.numpy())
    assert np.array_equal(ranks.cpu().numpy().astype(np.int64), lexsort_ranks(S.numpy(), keep, tid.numpy()))
    assert torch.equal(bits(scores.cpu()), bits(torch.gather(S, 1, tid)))
    listed = corpus.rank_topk(m, p, t, 256, exclude_ids=excl.to(DEV), eligible=ok.to(DEV))[1].cpu().numpy()
    r = ranks.cpu().numpy()
    for u, j in zip(*np.nonzero((r >= 0) & (r < 256))):
        assert listed[u, r[u, j]] == tid[u, j], (u, j)


def test_one_chunk_per_step():
    """fp16 at d = 64: a news row is one 128-byte chunk, a step one chunk (the ids of a step are loaded
    and used within the same chunk)."""
    U, K, d, N = 5, 32, 64, 600
    m, p, t, gen = random_users(64, U, K, d, N, torch.float16, dup=DUP)
    for st in ("weighted", "mean"):
        S = gpu_score_matrix(m, p, t, st)
        cand = torch.randint(0, N, (U, 300), generator=gen)
        got = corpus.score_pairs(m, p, t, cand.to(DEV), score_type=st).cpu()
        assert torch.equal(bits(got), bits(torch.gather(S, 1, cand))), st
        tid = torch.cat([torch.randint(0, N, (U, 5), generator=gen), torch.tensor([[0, N // 2, N - 1]]).expand(U, 3)], dim=1)
        ranks, _ = corpus.rank_of(m, p, t, tid.to(DEV), score_type=st)
        want = lexsort_ranks(S.numpy(), keep_mask(U, N), tid.numpy())
        assert np.array_equal(ranks.cpu().numpy().astype(np.int64), want), st


def test_evaluate_corpus():
    """Identical ranks for batch = 2 and batch >= U, equal to rank_of on encode_users' output with the
    histories excluded; the metrics are corpus_metrics' means of those ranks."""
    gen = torch.Generator().manual_seed(21)
    U, L, K, d, Dc, N, T = 5, 40, 32, 64, 96, 200, 4
    table = (torch.randn(N, d, generator=gen) / d ** 0.5).to(DEV)
    mask = (torch.arange(L)[None, :] >= torch.randint(0, L - 4, (U, 1), generator=gen)).to(DEV)
    hid = torch.randint(0, N, (U, L), generator=gen).int().to(DEV)
    pk = corpus.pack_encoder((torch.randn(Dc, d, generator=gen) / d ** 0.5).to(DEV), (torch.randn(K, Dc, generator=gen) * 0.3).to(DEV),
                             (torch.randn(d, d, generator=gen) / d ** 0.5).to(DEV), dtype=torch.float32)
    tid = torch.randint(0, N, (U, T), generator=gen)
    tid[1, 2:] = -1                                               # fewer targets for one user
    tid[2, 0] = hid[2, L - 1].item()                              # a target in the user's own history
    tid = tid.to(DEV)
    ok = (torch.rand(N, generator=gen) < 0.8).to(DEV)
    for elig in (None, ok):
        a, ma = corpus.evaluate_corpus(table, hid, mask, pk, tid, batch=2, eligible=elig)
        b, mb = corpus.evaluate_corpus(table, hid, mask, pk, tid, batch=U + 3, eligible=elig)
        assert torch.equal(a, b) and ma.keys() == mb.keys()
        assert all(ma[k] == mb[k] or (np.isnan(ma[k]) and np.isnan(mb[k])) for k in ma)
        mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
        seen = torch.where(mask, hid, -1)
        c, _ = corpus.rank_of(mui, proj, table, tid, exclude_ids=seen, eligible=elig)
        assert torch.equal(a, c)
        assert a[2, 0].item() == -1 and (a[1, 2:] == -1).all()
        # against the ranking kernels' list of the same users under the same filters
        listed = corpus.rank_topk(mui, proj, table, 256, exclude_ids=seen, eligible=elig)[1]
        for u, j in zip(*np.nonzero(a.cpu().numpy() >= 0)):
            assert listed[u, a[u, j]].item() == tid[u, j].item()
        survivors = (listed >= 0).sum(1)                          # N < 256: the list is complete
        want = corpus.corpus_metrics(a, survivors, ks=(5, 10))[1]
        assert set(ma) == {"recall@5", "recall@10", "hit@5", "hit@10", "ndcg@5", "ndcg@10", "mrr", "auc"}
        assert all(abs(ma[k] - want[k]) <= 1e-12 for k in want)
    c, _ = corpus.evaluate_corpus(table, hid, mask, pk, tid, exclude_history=False)
    d0, _ = corpus.rank_of(*corpus.encode_users(table, mask, pk, his_ids=hid), table, tid)
    assert torch.equal(c, d0)


@pytest.mark.parametrize("shape,k", [("small_f32", 256), ("mid_f16", 100), ("c5_f16", 100)])
def test_rescore_topk(shape, k):
    """Lists ranked with one set of user vectors, re-scored with another: per user, the list of
    rank_topk(news_ids=<its old ids>) with the new vectors, bit for bit (k = 256 > N: lists that end
    in (-inf, -1) entries); with a bitmap, the pruned list."""
    z = world(shape, "weighted")
    U, K, d, N, dtype = SHAPES[shape]
    old = corpus.rank_topk(z["m"], z["p"], z["t"], k)
    m2, p2, _, _ = random_users(99, U, K, d, 8, dtype)
    for ok in (None, z["ok"].to(DEV)):
        got = corpus.rescore_topk(old, m2, p2, z["t"], eligible=ok)
        assert got[0].shape == (U, k) and got[1].shape == (U, k)
        for u in range(U):
            ids = old[1][u][old[1][u] >= 0]
            want = corpus.rank_topk(m2[u:u + 1], p2[u:u + 1], z["t"], k, news_ids=ids, eligible=ok)
            assert torch.equal(bits(got[0][u:u + 1]), bits(want[0])) and torch.equal(got[1][u:u + 1], want[1]), u
    assert not torch.equal(got[1], old[1])                        # the new vectors rank them otherwise
