"""Diversity re-ranking on the device (miner_topk_diversify; corpus.diversify_topk / rank_topk_diverse)
— needs an MI355X. The reference project has no such stage: the yardstick is the definition of
include/miner_diversify.h restated in float64 by tests/diversify_ref.py.

* exact: a table whose rows hold exactly 16 entries of ±1 (G an exact integer in any summation order,
  sqrtf(16) = 4, sim = G / 16 exact) and scores that are multiples of 1/8 in [0, 8] with 0 and 8 in
  every row (minmax rel exact), at λ in {1/2, 1/4, 1}: every fp32 operation of the kernel is exact, so
  positions, ids, score bits and the objective's bits must equal ``greedy``'s — and ``greedy`` meets
  exact objective ties in every parametrisation with more than one entry (asserted), so the tie rule
  is what is tested. (A pool of one entry cannot hold both 0 and 8 nor a tie: it has the score 8.)
* random tables (normal, heavy-tailed and near-duplicate rows) under ``check``, which follows the
  kernel's prefix with the derived tolerance tol_obj.
* the edges, batch independence, λ = 1, and rank_topk_diverse against its two halves.
"""
import functools

import numpy as np
import pytest
import torch

import diversify_ref as ref
from miner_amd import corpus
from test_corpus_diversify_host import N_TABLE, random_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = N_TABLE
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
PATTERNS = np.array([[1] * 16, [1] * 8 + [-1] * 8, [1, -1] * 8, [-1] * 16], np.float64)


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def exact_table(d, zero_row=None, inf_row=None):
    """float64 [N, d], 16 entries of ±1 per row. Rows [0, 128): one of four sign patterns on one of
    up to four 16-column blocks — many identical rows (sim 1), opposite rows (sim −1) and orthogonal
    ones; rows [128, 320): random supports inside the first min(d, 64) columns (sims at every
    multiple of 1/16); the rest: random supports over all d columns."""
    g = np.random.default_rng(5)
    tab = np.zeros((N, d))
    nb = min(d // 16, 4)
    for n in range(N):
        if n < 128:
            b = n % nb
            tab[n, 16 * b:16 * b + 16] = PATTERNS[(n // 4) % 4]
        else:
            cols = g.choice(min(d, 64) if n < 320 else d, 16, replace=False)
            tab[n, cols] = g.choice([-1.0, 1.0], 16)
    if zero_row is not None:
        tab[zero_row] = 0.0
    if inf_row is not None:
        tab[inf_row, 3] = np.inf
    return tab


def exact_pools(U, P, seed):
    """scores fp32 [U,P] (multiples of 1/8 in [0, 8], two 8s and a 0 per row from P = 3 on), ids
    int64 [U,P] (half from the patterned rows, one id repeated), in no particular order."""
    g = np.random.default_rng(seed)
    vals = np.array([0, 0.125, 1, 1, 2.5, 4, 4, 4, 5.25, 6.875, 7, 8], np.float32)
    scores = g.choice(vals, (U, P))
    ids = np.where(g.random((U, P)) < 0.5, g.integers(0, 128, (U, P)), g.integers(0, N, (U, P)))
    for u in range(U):
        if P >= 3:
            a, b, c = g.choice(P, 3, replace=False)
            scores[u, a] = scores[u, b] = 8
            scores[u, c] = 0
            ids[u, b] = ids[u, (b + 1) % P]                       # one repeated id
        elif P == 2:
            scores[u] = [0, 8]
        else:
            scores[u] = 8
    return torch.from_numpy(scores), torch.from_numpy(ids)


def run(scores, ids, table, topk, lam, relevance):
    """(scores, ids, positions, objective) of the kernel, on the CPU."""
    out = corpus.diversify_topk((scores.to(DEV), ids.to(DEV)), table if table.is_cuda else table.to(DEV), topk, lam=lam,
                                relevance=relevance, return_positions=True, return_objective=True)
    assert [o.dtype for o in out] == [torch.float32, torch.int32, torch.int32, torch.float32]
    assert all(o.shape == (scores.shape[0], topk) for o in out)
    return [o.cpu() for o in out]


def assert_exact(got, want, what):
    ws, wi, wp, wo = want
    assert np.array_equal(got[2].numpy(), wp), (what, "positions", got[2][0, :8].tolist(), wp[0, :8].tolist())
    assert np.array_equal(got[1].numpy(), wi), (what, "ids")
    assert np.array_equal(got[0].numpy().view(np.uint32), ws.view(np.uint32)), (what, "score bits")
    assert np.array_equal(got[3].numpy().view(np.uint32), wo.astype(np.float32).view(np.uint32)), (what, "objective bits")


EXACT = [(dt, d, P) for dt in DTYPES for d in ((32, 64, 768) if dt == torch.float32 else (64, 768)) for P in (1, 31, 33, 256)]


@pytest.mark.parametrize("dtype,d,P", EXACT, ids=lambda v: str(v).replace("torch.", ""))
def test_exact_fixture_ties_and_arithmetic(dtype, d, P):
    tab64 = exact_table(d)
    table = torch.from_numpy(tab64).to(dtype).to(DEV)
    scores, ids = exact_pools(3, P, 100 + P)
    for topk in sorted({1, P}):
        for lam in (0.5, 0.25, 1.0):
            for relevance in ("minmax", "score"):
                stats = {}
                want = ref.greedy(scores, ids, tab64, topk, lam, relevance, stats)
                assert P == 1 or stats["ties"] > 0, "the fixture must make greedy break ties by position"
                assert_exact(run(scores, ids, table, topk, lam, relevance), want, (dtype, d, P, topk, lam, relevance))


RANDOM = [(dt, d, P) for dt in DTYPES for d in (64, 768, 1024) for P in (100, 256)]


@pytest.mark.parametrize("dtype,d,P", RANDOM, ids=lambda v: str(v).replace("torch.", ""))
def test_random_tables_under_check(dtype, d, P):
    scores, ids, table = random_inputs(11, dtype, d, P, 5)
    tab_dev = table.to(DEV)
    worst = 0.0
    for topk in sorted({10, 100, P}):
        for lam in (0.0, 0.3, 0.7):
            for relevance in ("minmax", "score"):
                got = run(scores, ids, tab_dev, topk, lam, relevance)
                worst = max(worst, ref.check(got, (scores, ids, table, topk, lam, relevance), dtype))
    print(f"diversify {dtype} d={d} P={P}: worst (float64 best - pick) / tol_obj = {worst:.3g}")


def test_edges():
    """One batch, P = topk = 100, on the exact table (so greedy is the yardstick, bit for bit): a row of
    all tails; 3 candidates among tails; NaN, +inf and -inf scores; ids -1, N and 2^31 - 1; a pool
    with the all-zero table row and the row that holds an inf; all scores equal (s_max == s_min)."""
    P, d = 100, 64
    zero_row, inf_row = 7, 9
    tab64 = exact_table(d, zero_row, inf_row)
    scores, ids = exact_pools(7, P, 41)
    scores[0] = float("-inf")
    ids[0] = -1
    scores[1, 3:] = float("-inf")
    ids[1, 3:] = -1
    scores[2, 5], scores[2, 6], scores[2, 7] = float("nan"), float("inf"), float("-inf")
    ids[3, 10], ids[3, 11], ids[3, 12] = -1, N, 2 ** 31 - 1
    ids[4, 20], ids[4, 21], ids[4, 22], ids[4, 23] = zero_row, inf_row, zero_row, inf_row
    scores[4, 20:24] = torch.tensor([8, 8, 7, 7])
    scores[5] = 2.5
    for dtype in DTYPES:
        table = torch.from_numpy(tab64).to(dtype).to(DEV)
        for lam, relevance in ((0.5, "minmax"), (0.25, "score"), (1.0, "minmax")):
            got = run(scores, ids, table, P, lam, relevance)
            want = ref.greedy(scores, ids, tab64, P, lam, relevance)
            assert_exact(got, want, (dtype, lam, relevance))
            ref.check(got, (scores, ids, tab64, P, lam, relevance), dtype)
            assert (got[2][0] == -1).all() and (got[1][0] == -1).all() and torch.isneginf(got[0][0]).all()
            assert (got[2][1, :3] >= 0).all() and (got[2][1, 3:] == -1).all()
            assert not set(got[2][2].tolist()) & {5, 6, 7} and (got[2][2, 97:] == -1).all()
            assert not set(got[2][3].tolist()) & {10, 11, 12}
            assert {20, 21, 22, 23} <= set(got[2][4].tolist())
    # narrower ids, as merge_topk takes them
    got16 = corpus.diversify_topk((scores.to(DEV), ids.clamp(max=N).to(torch.int16).to(DEV)), table, 10)
    got64 = corpus.diversify_topk((scores.to(DEV), ids.clamp(max=N).to(DEV)), table, 10)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got16, got64))


def test_non_default_stream():
    scores, ids, table = random_inputs(11, torch.float16, 768, 100, 5)
    want = run(scores, ids, table, 40, 0.7, "minmax")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        tab = table.to(DEV, non_blocking=False)
        got = corpus.diversify_topk((scores.to(DEV), ids.to(DEV)), tab, 40, return_positions=True, return_objective=True)
    side.synchronize()
    assert all(torch.equal(bits(a.cpu()), bits(b)) for a, b in zip(got, want))


def test_batch_independence():
    U = 300
    scores, ids, table = random_inputs(13, torch.float16, 64, 100, U)
    scores, ids = scores.clone(), ids.clone()
    scores[5, 50:] = float("-inf")                                # some half-empty and empty pools among them
    ids[5, 50:] = -1
    ids[6] = -1
    s, i, tab = scores.to(DEV), ids.to(DEV), table.to(DEV)
    kw = dict(lam=0.6, return_positions=True, return_objective=True)
    whole = corpus.diversify_topk((s, i), tab, 50, **kw)
    for step in (1, 7):
        parts = [corpus.diversify_topk((s[u:u + step], i[u:u + step]), tab, 50, **kw) for u in range(0, U, step)]
        for k, w in enumerate(whole):
            assert torch.equal(bits(torch.cat([p[k] for p in parts])), bits(w)), (step, k)


@functools.lru_cache(maxsize=None)
def users(dtype=torch.float16, U=6, K=8, d=64, seed=3):
    g = torch.Generator().manual_seed(seed)
    mui = torch.randn(U, K, d, generator=g).to(dtype).to(DEV)
    proj = (0.3 * torch.randn(U, K, d, generator=g)).to(dtype).to(DEV)
    table = random_inputs(17, dtype, d, 100, 1)[2].to(DEV)
    return mui, proj, table


def test_lambda_one_returns_the_ranked_prefix():
    mui, proj, table = users()
    lists = corpus.rank_topk(mui, proj, table, 64)
    for relevance in ("minmax", "score"):
        s, i, pos = corpus.diversify_topk(lists, table, 20, lam=1.0, relevance=relevance, return_positions=True)
        assert torch.equal(bits(s), bits(lists[0][:, :20])) and torch.equal(i, lists[1][:, :20])
        assert torch.equal(pos.cpu(), torch.arange(20, dtype=torch.int32).expand(6, 20))


def test_rank_topk_diverse_is_its_two_halves():
    mui, proj, table = users()
    U = mui.shape[0]
    g = torch.Generator().manual_seed(9)
    excl = torch.randint(0, N, (U, 12), generator=g).to(DEV)
    elig = (torch.rand(N, generator=g) < 0.8).to(DEV)
    bias = (0.5 * torch.randn(N, generator=g)).to(DEV)
    clus = (torch.arange(N) % 60).to(DEV)
    for kw in (dict(), dict(exclude_ids=excl, eligible=elig, news_bias=bias), dict(news_cluster=clus, cluster_cap=2),
               dict(score_type="max", exclude_ids=excl)):
        for topk, pool in ((10, None), (25, 60), (40, 40)):
            got = corpus.rank_topk_diverse(mui, proj, table, topk, pool=pool, lam=0.4, **kw)
            lists = corpus.rank_topk(mui, proj, table, min(256, 4 * topk) if pool is None else pool, **kw)
            want = corpus.diversify_topk(lists, table, topk, lam=0.4)
            assert len(got) == 2 and all(torch.equal(bits(a), bits(b)) for a, b in zip(got, want)), (kw.keys(), topk)
            ids = got[1].cpu()
            assert (ids >= 0).all()
            if "exclude_ids" in kw:
                for u in range(U):
                    assert not set(ids[u].tolist()) & set(excl[u].tolist())
            if "eligible" in kw:
                assert elig.cpu()[ids.long()].all()
            if "news_cluster" in kw:                              # a subset of a capped pool keeps its caps
                c = clus.cpu()[ids.long()]
                assert max(int(torch.bincount(c[u]).max()) for u in range(U)) <= 2
    # the default is a different page than the ranked prefix (the re-ranking does something here)
    assert not torch.equal(corpus.rank_topk_diverse(mui, proj, table, 10, lam=0.4)[1], corpus.rank_topk(mui, proj, table, 10)[1])


def test_rank_topk_diverse_with_interests():
    mui, proj, table = users()
    for kw in (dict(), dict(interest_cap=6)):
        s, i, gi = corpus.rank_topk_diverse(mui, proj, table, 12, lam=0.5, return_interest=True, **kw)
        lists = corpus.rank_topk(mui, proj, table, 48, return_interest=True, **kw)
        ws, wi, wg, wp = corpus.diversify_topk(lists, table, 12, lam=0.5, return_positions=True)
        assert torch.equal(bits(s), bits(ws)) and torch.equal(i, wi) and torch.equal(gi, wg) and gi.dtype == torch.int32
        assert torch.equal(wg, lists[2].gather(1, wp.long()))
        _, pair_g = corpus.score_pairs(mui, proj, table, i, return_interest=True)
        assert torch.equal(gi, pair_g)
        if kw:
            assert max(int(torch.bincount(gi[u].cpu()).max()) for u in range(mui.shape[0])) <= 6
    # a short pool: the interests' tail is -1
    few = torch.arange(5, device=DEV)
    s, i, gi = corpus.rank_topk_diverse(mui, proj, table, 8, pool=8, news_ids=few, return_interest=True)
    assert (i[:, 5:] == -1).all() and (gi[:, 5:] == -1).all() and (gi[:, :5] >= 0).all() and torch.isneginf(s[:, 5:]).all()
