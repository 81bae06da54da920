"""The ranker's subset form and the device-side list merge (miner_rank_topk_subset, miner_topk_merge;
corpus.rank_topk / rank_corpus news_ids=, merge_topk, update_topk) — needs an MI355X.

The subset form is never compared with itself alone. Its yardsticks are
* the bitmap form (``eligible=`` "n is in the list", the parent commit's kernels), bit for bit, and
* the oracle (oracle.corpus_oracle.corpus_scores) with the non-members at -inf, through
  check_filtered of tests/test_gpu_corpus_filter.py (copied) at that file's bars: fp32
  1e-5·|ref| + 1e-5·rms, 16-bit 2e-4 / 2e-4.
merge_topk is checked against a numpy lexsort written here.
"""
import numpy as np
import pytest
import torch

from miner_amd import corpus
from oracle import corpus_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_TOL = dict(rtol=1e-5, rms_floor=1e-5)          # the bars of tests/test_gpu_corpus_filter.py
RANK16_TOL = dict(rtol=2e-4, rms_floor=2e-4)


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


def check_filtered(ts, ti, ref_scores, keep, k, tol):
    """check_filtered of tests/test_gpu_corpus_filter.py: the list against ref_scores [U,N] (float64)
    with the filtered entries at -inf; n_ok = min(k, survivors), every returned id a survivor."""
    ts, ti = ts.cpu().numpy().astype(np.float64), ti.cpu().numpy().astype(np.int64)
    U, N = ref_scores.shape
    rms = float(np.sqrt(np.mean(ref_scores ** 2)))
    bound = lambda x: tol["rtol"] * np.abs(x) + tol["rms_floor"] * rms
    masked = np.where(keep, ref_scores, -np.inf)
    for u in range(U):
        n_ok = min(k, int(keep[u].sum()))
        assert (ti[u, n_ok:] == -1).all() and np.isneginf(ts[u, n_ok:]).all(), f"user {u}: tail"
        if n_ok == 0:
            continue
        ids = ti[u, :n_ok]
        assert len(set(ids.tolist())) == n_ok and (ids >= 0).all() and (ids < N).all()
        assert keep[u, ids].all(), f"user {u}: a filtered news was returned"
        true = ref_scores[u, ids]
        assert (np.abs(ts[u, :n_ok] - true) <= bound(true)).all(), f"user {u}: returned scores off"
        assert (np.diff(ts[u, :n_ok]) <= 0).all(), f"user {u}: not sorted"
        kth = true.min()
        rest = np.delete(masked[u], ids)
        assert (rest <= kth + 2 * bound(kth)).all(), f"user {u}: a news outside the top-k beats it"


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


def oracle_scores(m, p, t, score_type="weighted"):
    return co.corpus_scores(m.float().cpu(), p.float().cpu(), t.float().cpu(), score_type).double().numpy()


def member_mask(ids, N):
    """bool [N] (CPU): news n is in the id list (entries outside [0, N) name nothing)."""
    ids = torch.as_tensor(ids, dtype=torch.int64)
    mask = torch.zeros(N, dtype=torch.bool)
    mask[ids[(ids >= 0) & (ids < N)]] = True
    return mask


def raw_list(ids, N):
    """The ids as given — any order, no canonicalisation — for the kernel itself (distinct, in range)."""
    return corpus.NewsIdList(torch.as_tensor(ids, dtype=torch.int32).to(DEV).contiguous(), N)


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.fixture(scope="module")
def small():
    """U = 5, K = 32, d = 64, N = 200, fp32: users, histories with padded slots, a random 50 % id list,
    a further bitmap, and the oracle's scores per score type."""
    U, K, d, N = 5, 32, 64, 200
    m, p, t, gen = random_users(11, U, K, d, N, torch.float32)
    hist = torch.randint(0, N, (U, 40), generator=gen)
    hist[:, :7] = -1
    ids = torch.nonzero(torch.rand(N, generator=gen) < 0.5)[:, 0]
    ok2 = torch.rand(N, generator=gen) < 0.6
    ref = {st: oracle_scores(m, p, t, st) for st in ("weighted", "max", "mean")}
    return dict(U=U, N=N, m=m, p=p, t=t, hist=hist, ids=ids, ok2=ok2, ref=ref)


@pytest.fixture(scope="module")
def mid():
    """U = 3, K = 64, d = 128, N = 1000 (three full 256-steps + 232 rows) per dtype, with the oracle."""
    out = {}
    for dtype in (torch.float16, torch.float32):
        m, p, t, _ = random_users(31, 3, 64, 128, 1000, dtype)
        out[dtype] = dict(m=m, p=p, t=t, ref=oracle_scores(m, p, t), tol=F32_TOL if dtype == torch.float32 else RANK16_TOL)
    return out


@pytest.mark.parametrize("score_type", ["weighted", "max", "mean"])
def test_small_table_every_score_type(small, score_type):
    """The id list against eligible= bitwise and against the oracle; with the histories as
    exclude_ids; with a further bitmap on top (the intersection)."""
    z = small
    U, N, m, p, t = z["U"], z["N"], z["m"], z["p"], z["t"]
    ids, member = z["ids"].to(DEV), member_mask(z["ids"], N)
    hist = z["hist"].to(DEV)
    cases = {"list": (None, None), "history": (hist, None), "bitmap": (None, z["ok2"]), "both": (hist, z["ok2"])}
    for name, (excl, ok2) in cases.items():
        a = corpus.rank_topk(m, p, t, 256, score_type=score_type, news_ids=ids, exclude_ids=excl,
                             eligible=None if ok2 is None else ok2.to(DEV))
        both = member if ok2 is None else member & ok2
        b = corpus.rank_topk(m, p, t, 256, score_type=score_type, exclude_ids=excl, eligible=both.to(DEV))
        assert same(a, b), (score_type, name)
        keep = keep_mask(U, N, None if excl is None else z["hist"].numpy(), both.numpy())
        check_filtered(a[0], a[1], z["ref"][score_type], keep, 256, F32_TOL)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 700, 1000])
def test_steps_and_partial_steps(mid, dtype, M):
    """List lengths around the 256-position step; the lists hold the table's first and last news
    (M = 1: each alone), in a shuffled order given to the kernel as it is."""
    z = mid[dtype]
    U, N, k = 3, 1000, 100
    gen = torch.Generator().manual_seed(M)
    if M == 1:
        lists = [torch.tensor([0]), torch.tensor([N - 1])]
    else:
        inner = torch.randperm(N - 2, generator=gen)[:M - 2] + 1
        ids = torch.cat([torch.tensor([0, N - 1]), inner])
        lists = [ids[torch.randperm(M, generator=gen)]]
    for ids in lists:
        assert len(set(ids.tolist())) == M
        member = member_mask(ids, N)
        a = corpus.rank_topk(z["m"], z["p"], z["t"], k, news_ids=raw_list(ids, N))
        b = corpus.rank_topk(z["m"], z["p"], z["t"], k, eligible=member.to(DEV))
        assert same(a, b), M
        check_filtered(a[0], a[1], z["ref"], keep_mask(U, N, None, member.numpy()), k, z["tol"])
        if M < k:                                   # every member, then the tail
            got = a[1].cpu()
            assert ((got >= 0).sum(1) == M).all()
            assert all(set(got[u, :M].tolist()) == set(ids.tolist()) for u in range(U))


@pytest.mark.parametrize("split", ["0", "1"])
def test_one_chunk_per_step(split, monkeypatch):
    """fp16 at d = 64: a news row is one 128-byte chunk, so a step's ids are loaded and used within the
    same chunk (no later chunk's wait in between). U = 5, N = 600, M = 300 in a shuffled order."""
    monkeypatch.setenv("MINER_RK_SPLIT", split)
    U, K, d, N, M, k = 5, 32, 64, 600, 300, 50
    m, p, t, gen = random_users(64, U, K, d, N, torch.float16)
    ids = torch.randperm(N, generator=gen)[:M]
    member = member_mask(ids, N)
    for st in ("weighted", "mean"):
        a = corpus.rank_topk(m, p, t, k, score_type=st, news_ids=raw_list(ids, N))
        b = corpus.rank_topk(m, p, t, k, score_type=st, eligible=member.to(DEV))
        assert same(a, b), st
        check_filtered(a[0], a[1], oracle_scores(m, p, t, st), keep_mask(U, N, None, member.numpy()), k, RANK16_TOL)


def test_order_duplicates_junk(mid):
    """Through the wrapper: a permuted list, one with repeats and one with -1, N and 2^31 - 1 mixed
    in all return the plain list's result, which is the bitmap form's."""
    z = mid[torch.float16]
    N, k = 1000, 100
    gen = torch.Generator().manual_seed(3)
    plain = torch.sort(torch.randperm(N, generator=gen)[:300])[0]
    want = corpus.rank_topk(z["m"], z["p"], z["t"], k, eligible=member_mask(plain, N).to(DEV))
    perm = plain[torch.randperm(300, generator=gen)]
    rep = torch.cat([perm, plain[:120], perm[:7]])
    junk = torch.cat([torch.tensor([-1, N, 2 ** 31 - 1]), perm, torch.tensor([N + 5, -(2 ** 31), N])])
    for name, ids in (("plain", plain), ("permuted", perm), ("repeats", rep), ("junk", junk),
                      ("int32", junk.to(torch.int32)), ("canonical", corpus.canonical_news_ids(rep.to(DEV), N))):
        got = corpus.rank_topk(z["m"], z["p"], z["t"], k, news_ids=ids if name == "canonical" else ids.to(DEV))
        assert same(got, want), name
        assert (got[1] < N).all()
    check_filtered(want[0], want[1], z["ref"], keep_mask(3, N, None, member_mask(plain, N).numpy()), k, z["tol"])


@pytest.mark.parametrize("split,U,N,M", [("1", 70, 600, 300), ("0", 515, 300, 150)])
def test_several_tiles_per_workgroup(split, U, N, M, monkeypatch):
    """More user tiles than workgroups (split: 35 tiles over 32 tile slots; unsplit: 258 tiles over
    256 workgroups): the issue side's ids cross tile boundaries. 50 table rows are duplicated and
    both copies are in the list: exact ties across steps and slices. Oracle, and split == unsplit."""
    K, d, k = 32, 64, 20
    m, p, t, gen = random_users(U + N, U, K, d, N, torch.float32, dup=50)
    ref = oracle_scores(m, p, t)
    rest = torch.tensor([n for n in range(N) if not (n < 50 or N // 2 <= n < N // 2 + 50)])
    ids = torch.cat([torch.arange(50), torch.arange(N // 2, N // 2 + 50), rest[torch.randperm(len(rest), generator=gen)[:M - 100]]])
    ids = ids[torch.randperm(M, generator=gen)]
    assert len(set(ids.tolist())) == M
    monkeypatch.setenv("MINER_RK_SPLIT", split)
    a = corpus.rank_topk(m, p, t, k, news_ids=raw_list(ids, N))
    check_filtered(a[0], a[1], ref, keep_mask(U, N, None, member_mask(ids, N).numpy()), k, F32_TOL)
    monkeypatch.setenv("MINER_RK_SPLIT", "0" if split == "1" else "1")
    b = corpus.rank_topk(m, p, t, k, news_ids=raw_list(ids, N))
    assert same(a, b)
    c = corpus.rank_topk(m, p, t, k, eligible=member_mask(ids, N).to(DEV))
    assert same(a, c)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("U,N,M,topk", [(37, 5000, 1200, 7), (3, 200, 90, 256)])
def test_compile_time_instantiations(dtype, U, N, M, topk, monkeypatch):
    """K = 64, d = 768 (16-bit: the chunk count and K compile-time): the subset form must take the
    instantiation the bitmap form takes — equal bit for bit, under both MINER_RK_SPLIT settings."""
    K, d = 64, 768
    gen = torch.Generator().manual_seed(U + N)
    table = torch.randn(N, d, generator=gen) / d ** 0.5
    table[N // 2:N // 2 + 50] = table[:50]
    mui = (torch.randn(U, K, d, generator=gen) / 4).to(DEV, dtype)
    proj = (torch.randn(U, K, d, generator=gen) / 4).to(DEV, dtype)
    tab = table.to(DEV, dtype)
    ids = torch.randperm(N, generator=gen)[:M]
    ok = member_mask(ids, N).to(DEV)
    for st in ("weighted", "max"):
        outs = []
        for split in ("1", "0"):
            monkeypatch.setenv("MINER_RK_SPLIT", split)
            a = corpus.rank_topk(mui, proj, tab, topk, score_type=st, news_ids=raw_list(ids, N))
            b = corpus.rank_topk(mui, proj, tab, topk, score_type=st, eligible=ok)
            assert same(a, b), (st, split)
            outs.append(a)
        assert same(outs[0], outs[1]), st
        assert ((outs[0][1] >= 0).sum(1) == min(topk, M)).all()


def test_empty_list(small):
    """M = 0 — an empty tensor, or nothing but ids outside the table: all (-inf, -1), no error."""
    z = small
    for ids in (torch.empty(0, dtype=torch.int64), torch.tensor([-1, z["N"], 2 ** 31 - 1])):
        ts, ti = corpus.rank_topk(z["m"], z["p"], z["t"], 9, news_ids=ids.to(DEV))
        assert ts.shape == (z["U"], 9) and (ti == -1).all() and torch.isneginf(ts).all()


def ref_merge(a, b, topk, ok=None):
    """numpy: per user the union of the valid entries (b's entry for an id in both), the eligible
    ones, ordered by (score desc, id asc) with a lexsort, cut / padded to topk."""
    a_s, a_i, b_s, b_i = (x.cpu().numpy() for x in (*a, *b))
    U = a_s.shape[0]
    out_s = np.full((U, topk), -np.inf, np.float32)
    out_i = np.full((U, topk), -1, np.int32)
    for u in range(U):
        d = {int(i): s for s, i in zip(a_s[u], a_i[u]) if i >= 0}
        d.update({int(i): s for s, i in zip(b_s[u], b_i[u]) if i >= 0})
        if ok is not None:
            d = {i: s for i, s in d.items() if ok[i]}
        ids = np.array(sorted(d), np.int64)
        sc = np.array([d[i] for i in ids], np.float32)
        order = np.lexsort((ids, -sc.astype(np.float64)))[:topk]
        out_s[u, :len(order)] = sc[order]
        out_i[u, :len(order)] = ids[order]
    return out_s, out_i


def make_list(gen, U, k, n_ids, tail):
    """Unsorted rows of k distinct ids of [0, n_ids) with scores from a few values (ties across the
    lists), the last `tail` entries (-inf, -1)."""
    ids = torch.stack([torch.randperm(n_ids, generator=gen)[:k] for _ in range(U)]).to(torch.int32)
    sc = torch.randint(-6, 7, (U, k), generator=gen).float() / 4
    if tail:
        ids[:, k - tail:] = -1
        sc[:, k - tail:] = float("-inf")
    return sc.to(DEV), ids.to(DEV)


@pytest.mark.parametrize("ka,kb,topk", [(256, 256, 256), (7, 100, 100)])
def test_merge_topk_against_lexsort(ka, kb, topk):
    """Lists that end in tails, ids in both lists with different scores (b's wins), equal scores
    across the lists (lower id first), a bitmap that removes entries from both, two empty lists."""
    U, n_ids = 5, 400
    gen = torch.Generator().manual_seed(ka + kb)
    a = make_list(gen, U, ka, n_ids, tail=ka // 4)
    b = make_list(gen, U, kb, n_ids, tail=kb // 5)
    ai, bi = a[1].cpu(), b[1].cpu()
    shared = [set(ai[u][ai[u] >= 0].tolist()) & set(bi[u][bi[u] >= 0].tolist()) for u in range(U)]
    assert any(shared)                                            # ids in both lists ...
    u0 = next(u for u in range(U) if shared[u])
    n0 = sorted(shared[u0])[0]                                    # ... one of them made to differ for certain
    a[0][u0, (ai[u0] == n0).nonzero()[0, 0]] = 5.0
    b[0][u0, (bi[u0] == n0).nonzero()[0, 0]] = -5.0
    ok = torch.rand(n_ids, generator=gen) < 0.6
    for elig, k in ((None, topk), (ok, topk), (None, None), (ok, 3)):
        got = corpus.merge_topk(a, b, k, eligible=None if elig is None else elig.to(DEV))
        k = max(ka, kb) if k is None else k
        es, ei = ref_merge(a, b, k, None if elig is None else elig.numpy())
        assert got[0].shape == (U, k) and got[1].dtype == torch.int32
        assert np.array_equal(got[1].cpu().numpy(), ei), (ka, kb, k, elig is not None)
        assert np.array_equal(got[0].cpu().numpy(), es), (ka, kb, k, elig is not None)
    es, ei = ref_merge(a, b, topk)
    row = ei[u0].tolist()
    assert n0 not in row or es[u0, row.index(n0)] == -5.0          # b's score, not a's
    # the packed form of the bitmap
    got = corpus.merge_topk(a, b, topk, eligible=corpus.pack_eligible(ok.to(DEV)))
    es, ei = ref_merge(a, b, topk, ok.numpy())
    assert np.array_equal(got[1].cpu().numpy(), ei) and np.array_equal(got[0].cpu().numpy(), es)
    # two empty lists
    e = (torch.full((U, ka), float("-inf"), device=DEV), torch.full((U, ka), -1, dtype=torch.int32, device=DEV))
    f = (torch.full((U, kb), float("-inf"), device=DEV), torch.full((U, kb), -1, dtype=torch.int32, device=DEV))
    ts, ti = corpus.merge_topk(e, f, topk)
    assert (ti == -1).all() and torch.isneginf(ts).all()
    # one empty list: the other one, sorted
    got = corpus.merge_topk(e, b, topk)
    es, ei = ref_merge(e, b, topk)
    assert np.array_equal(got[1].cpu().numpy(), ei) and np.array_equal(got[0].cpu().numpy(), es)


@pytest.mark.parametrize("overlap", [False, True])
def test_incremental_identity(mid, overlap):
    """merge_topk(rank(A), rank(B)) == rank(A ∪ B) == update_topk(rank(A), B), bit for bit — the
    union ranked by the bitmap form —, for disjoint and overlapping sets, with exclude_ids, and with
    an eligible that expires some of A (|A| <= topk there, so rank(A) holds all of A)."""
    z = mid[torch.float16]
    m, p, t, ref = z["m"], z["p"], z["t"], z["ref"]
    U, N, k = 3, 1000, 100
    gen = torch.Generator().manual_seed(8 + overlap)
    perm = torch.randperm(N, generator=gen)
    A, B = perm[:300], perm[200:500] if overlap else perm[300:500]
    union = member_mask(torch.cat([A, B]), N)
    excl = torch.from_numpy(np.argsort(-ref, axis=1)[:, :30].copy())           # every user's best 30 news
    for ex in (None, excl.to(DEV)):
        ra = corpus.rank_topk(m, p, t, k, news_ids=A.to(DEV), exclude_ids=ex)
        rb = corpus.rank_topk(m, p, t, k, news_ids=B.to(DEV), exclude_ids=ex)
        want = corpus.rank_topk(m, p, t, k, eligible=union.to(DEV), exclude_ids=ex)
        assert same(corpus.merge_topk(ra, rb, k), want)
        assert same(corpus.update_topk(ra, m, p, t, B.to(DEV), exclude_ids=ex), want)
        assert same(corpus.rank_topk(m, p, t, k, news_ids=torch.cat([A, B]).to(DEV), exclude_ids=ex), want)
        check_filtered(want[0], want[1], ref, keep_mask(U, N, None if ex is None else excl.numpy(), union.numpy()), k, z["tol"])
    # expiry: a short A (80 <= topk ids), a third of it and some of B no longer eligible
    A = perm[:80]
    elig = torch.rand(N, generator=gen) < 0.7
    assert 0 < int((~elig[A]).sum()) < 80
    ra = corpus.rank_topk(m, p, t, k, news_ids=A.to(DEV))
    assert ((ra[1] >= 0).sum(1) == 80).all()
    got = corpus.update_topk(ra, m, p, t, B.to(DEV), eligible=elig.to(DEV))
    alive = member_mask(torch.cat([A, B]), N) & elig
    want = corpus.rank_topk(m, p, t, k, eligible=alive.to(DEV))
    assert same(got, want)
    assert not (~elig)[got[1][got[1] >= 0].long().cpu()].any()


def test_rank_corpus_news_ids():
    """rank_corpus(news_ids=...): identical lists for batch = 2 and batch = U, equal to eligible=."""
    gen = torch.Generator().manual_seed(21)
    U, L, K, d, Dc, N = 5, 40, 32, 64, 96, 200
    table = (torch.randn(N, d, generator=gen) / d ** 0.5).to(DEV)
    mask = (torch.arange(L)[None, :] >= torch.randint(0, L - 4, (U, 1), generator=gen)).to(DEV)
    hid = torch.randint(0, N, (U, L), generator=gen).int().to(DEV)
    pk = corpus.pack_encoder((torch.randn(Dc, d, generator=gen) / d ** 0.5).to(DEV), (torch.randn(K, Dc, generator=gen) * 0.3).to(DEV),
                             (torch.randn(d, d, generator=gen) / d ** 0.5).to(DEV), dtype=torch.float32)
    ids = torch.randperm(N, generator=gen)[:90]
    a = corpus.rank_corpus(table, hid, mask, pk, 30, news_ids=ids.to(DEV), exclude_history=True, batch=2)
    b = corpus.rank_corpus(table, hid, mask, pk, 30, news_ids=ids.to(DEV), exclude_history=True, batch=U)
    c = corpus.rank_corpus(table, hid, mask, pk, 30, eligible=member_mask(ids, N).to(DEV), exclude_history=True, batch=U)
    assert same(a, b) and same(b, c)
    assert member_mask(ids, N)[b[1][b[1] >= 0].long().cpu()].all()


def test_argument_errors(small):
    z = small
    U, N, m, p, t = z["U"], z["N"], z["m"], z["p"], z["t"]
    with pytest.raises(ValueError):
        corpus.rank_topk(m, p, t, 5, news_ids=torch.zeros(3, 2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        corpus.rank_topk(m, p, t, 5, news_ids=torch.zeros(3, device=DEV))
    with pytest.raises(ValueError):
        corpus.rank_topk(m, p, t, 5, news_ids=corpus.canonical_news_ids(z["ids"].to(DEV), N + 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        corpus.rank_topk(m, p, t, 5, news_ids=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        corpus.canonical_news_ids(torch.zeros(3, dtype=torch.int64), N)
    ls = lambda u, k, dev=DEV: (torch.zeros(u, k, device=dev), torch.zeros(u, k, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        corpus.merge_topk(ls(U, 10), ls(U + 1, 10))
    with pytest.raises(ValueError):
        corpus.merge_topk(ls(U, 257), ls(U, 10))
    with pytest.raises(ValueError):
        corpus.merge_topk(ls(U, 10), ls(U, 10), 257)
    with pytest.raises(ValueError):
        corpus.merge_topk(ls(U, 10), (torch.zeros(U, 10, device=DEV), torch.zeros(U, 10, device=DEV)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        corpus.merge_topk(ls(U, 10, "cpu"), ls(U, 10))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        corpus.update_topk(ls(U, 10, "cpu"), m, p, t, z["ids"].to(DEV))
