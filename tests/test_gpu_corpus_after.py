"""Keyset cursors and deep lists (miner_rank_topk_after; corpus.rank_topk / rank_corpus with after=,
corpus.start_cursor / page_cursor / rank_topk_deep) — needs an MI355X.

The cursor form is never compared with itself alone. Its yardsticks are
* A, exact: S_gpu [U, N] of the UNCURSORED ranking kernels (base.world / base.gpu_score_matrix), plus
  bias[group] in torch fp32 where a prior is used. The expected list is made on the CPU:
  numpy.lexsort((ids, -S[u])) over the filters' survivors (base.keep_mask) with NaN dropped, the
  entries strictly after the cursor in that order (a lower score, or an equal one — a float compare —
  with a higher id), the first topk, then (-inf, -1). Ids must be equal and scores bit for bit.
* B: every returned score within base's bar of oracle.corpus_oracle's score for that id (fp32
  1e-5·|ref| + 1e-5·rms, 16-bit 2e-4 / 2e-4; with a prior, the prior added in float64 and one fp32
  rounding of the sum, 2^-23·|sum|, allowed on top), and the order non-increasing with ties by id.
The worlds, shapes and tables are those of tests/test_gpu_corpus_rankof.py / _bias.py: every table
repeats its rows [0, 8) at [N/2, N/2 + 8), exact ties that a cursor must split by id.
"""
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
INF = float("inf")
NAN = float("nan")
BIG = 2 ** 31 - 1
bits = base.bits


def orders(S, keep):
    """Per user the ids of the survivors (NaN dropped) in the ranker's order: score desc, id asc."""
    Snp = S.numpy()
    out = []
    for u in range(S.shape[0]):
        ids = np.flatnonzero(keep[u] & ~np.isnan(Snp[u]))
        out.append(ids[np.lexsort((ids, -Snp[u, ids].astype(np.float64)))])
    return out


def lists_after(S, keep, cur, topk, order=None):
    """Yardstick A: per user the entries of its order strictly after the cursor, the first topk, the tail."""
    U = S.shape[0]
    order = orders(S, keep) if order is None else order
    Snp = S.numpy()
    es = torch.full((U, topk), -INF)
    ei = torch.full((U, topk), -1, dtype=torch.int32)
    for u in range(U):
        o = order[u]
        if cur is not None:
            cs, ci = np.float32(cur[0][u]), int(cur[1][u])
            sc = Snp[u, o]
            o = o[(sc < cs) | ((sc == cs) & (o > ci))]           # a NaN cursor score: nothing
        o = o[:topk]
        if len(o):
            idx = torch.from_numpy(o)
            es[u, :len(o)] = S[u, idx]
            ei[u, :len(o)] = idx.int()
    return es, ei


def same(got, want, what):
    gs, gi = got[0].cpu(), got[1].cpu()
    assert gi.dtype == torch.int32 and gs.dtype == torch.float32 and gs.shape == want[0].shape, what
    assert torch.equal(gi, want[1]), (what, np.argwhere((gi != want[1]).numpy())[:5].tolist())
    assert torch.equal(bits(gs), bits(want[0])), what


def check_a(got, S, keep, cur, topk, what):
    same(got, lists_after(S, keep, cur, topk), what)


def check_b(got, ref, tol, what, prior=None):
    """Yardstick B; ``ref`` float64 [U, N] holds the oracle's scores, ``prior`` float64 [U, N] what
    the call adds to them (the bar is the unbiased score's, plus one fp32 rounding of the sum)."""
    gs, gi = got[0].cpu().double().numpy(), got[1].cpu().long().numpy()
    rms = float(np.sqrt(np.mean(ref ** 2)))
    add = np.zeros_like(ref) if prior is None else prior
    for u in range(gs.shape[0]):
        n = gi[u][gi[u] >= 0]
        s = gs[u][:len(n)]
        assert (gi[u][len(n):] == -1).all() and np.isneginf(gs[u][len(n):]).all(), what
        r = ref[u, n]
        bound = tol["rtol"] * np.abs(r) + tol["rms_floor"] * rms + EPS * np.abs(s)
        assert (np.abs(s - (r + add[u, n])) <= bound).all(), what
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (n[:-1] < n[1:]))).all(), what


def cursor_kw(cur, dtype=torch.int64):
    return dict(after=(torch.as_tensor(cur[0], dtype=torch.float32).to(DEV), torch.as_tensor(cur[1]).to(DEV, dtype)))


def chain(m, p, t, k, npages, kw, first=None):
    """npages pages of k chained with page_cursor from start_cursor (or ``first``), side by side, on
    the device; nothing is read back in between."""
    cur = corpus.start_cursor(m.shape[0], DEV) if first is None else first
    ps, pi = [], []
    for _ in range(npages):
        page = corpus.rank_topk(m, p, t, k, after=cur, **kw)
        cur = corpus.page_cursor(page)
        ps.append(page[0])
        pi.append(page[1])
    return torch.cat(ps, dim=1), torch.cat(pi, dim=1)


def combos_of(z, score_type):
    """(name, keyword arguments, S, prior float64 or None, keep) of every form a cursor composes with."""
    U, N = z["U"], z["N"]
    gen = torch.Generator().manual_seed(3 * N + U)
    sub, inside = biased.subset_ids(gen, N)
    excl, ok = z["hist"], z["ok"]
    pkw = biased.prior_kw(z)
    pb = z["bias"][z["group"]].double().numpy()
    st = dict(score_type=score_type)
    return [
        ("plain", dict(**st), z["S"], None, base.keep_mask(U, N)),
        ("excl", dict(exclude_ids=excl.to(DEV), **st), z["S"], None, base.keep_mask(U, N, excl.numpy())),
        ("bitmap", dict(eligible=ok.to(DEV), **st), z["S"], None, base.keep_mask(U, N, None, ok.numpy())),
        ("packed", dict(eligible=corpus.pack_eligible(ok.to(DEV)), **st), z["S"], None, base.keep_mask(U, N, None, ok.numpy())),
        ("subset", dict(news_ids=sub.to(DEV), **st), z["S"], None, base.keep_mask(U, N) & inside[None, :]),
        ("prior", dict(**pkw, **st), z["Sb"], pb, base.keep_mask(U, N)),
        ("all", dict(exclude_ids=excl.to(DEV), eligible=ok.to(DEV), news_ids=sub.to(DEV), **pkw, **st), z["Sb"], pb,
         base.keep_mask(U, N, excl.numpy(), ok.numpy()) & inside[None, :]),
    ]


world = biased.world


def test_the_new_surface_exists():
    assert hasattr(_lib.lib(), "miner_rank_topk_after")
    for name in ("start_cursor", "page_cursor", "rank_topk_deep", "rank_topk"):
        assert callable(getattr(corpus, name)), name
    s, i = corpus.start_cursor(3, DEV)
    assert s.dtype == torch.float32 and i.dtype == torch.int32 and s.device.type == "cuda"
    assert s.tolist() == [INF] * 3 and i.tolist() == [-1] * 3


@pytest.mark.parametrize("shape,score_type", base.CASES)
def test_paging_reproduces_the_ranking(shape, score_type, monkeypatch):
    """k = 1, 7, 100 and 256 under every form: the pages chained from start_cursor, two pages past
    exhaustion, concatenate to the complete lexsort and then stay empty; split and unsplit agree."""
    z = world(shape, score_type)
    U, N = z["U"], z["N"]
    for name, kw, S, prior, keep in combos_of(z, score_type):
        order = orders(S, keep)
        longest = max(len(o) for o in order)
        for k in (1, 7, 100, 256):
            npages = -(-longest // k) + 2
            want = lists_after(S, keep, None, npages * k, order)
            assert (want[1][:, -2 * k:] == -1).all()              # the last two pages are past every list's end
            got = {}
            for split in ("0", "1"):
                monkeypatch.setenv("MINER_RK_SPLIT", split)
                got[split] = chain(z["m"], z["p"], z["t"], k, npages, kw)
                same(got[split], want, (name, k, split))
            assert torch.equal(got["0"][1], got["1"][1]) and torch.equal(bits(got["0"][0]), bits(got["1"][0])), (name, k)
            if k == 100:
                check_b(got["0"], z["ref"], z["tol"], (name, k), prior)


@pytest.mark.parametrize("shape", ["small_f32", "mid_f16"])
def test_exact_ties(shape):
    """Rows n and N/2 + n (n < 8) score the same: a cursor at the lower id makes the page begin with
    the higher id, a cursor at the higher id lists neither."""
    z = world(shape, "weighted")
    U, N, S = z["U"], z["N"], z["S"]
    keep = base.keep_mask(U, N)
    for n in range(DUP):
        lo, hi = n, N // 2 + n
        assert torch.equal(bits(S[:, lo]), bits(S[:, hi]))
        for k in (1, 10):
            for dtype in (torch.int64, torch.int32):
                cur = (S[:, lo].clone(), torch.full((U,), lo))
                got = corpus.rank_topk(z["m"], z["p"], z["t"], k, **cursor_kw(cur, dtype))
                check_a(got, S, keep, cur, k, ("lower", n, k))
                assert (got[1][:, 0].cpu() == hi).all()
                cur = (S[:, lo].clone(), torch.full((U,), hi))
                got = corpus.rank_topk(z["m"], z["p"], z["t"], k, **cursor_kw(cur, dtype))
                check_a(got, S, keep, cur, k, ("higher", n, k))
                gi = got[1].cpu()
                assert not (gi == lo).any() and not (gi == hi).any()


@pytest.mark.parametrize("shape", ["small_f32", "c5_f16"])
def test_cursor_ids_that_are_not_listable(shape):
    """The cursor is a position in the order: ids that are excluded, ineligible, outside the subset,
    negative or past the table, at the score of a listed news r — an id below r lists r first, an id
    above it does not list r."""
    z = world(shape, "weighted")
    U, N = z["U"], z["N"]
    name, kw, S, prior, keep = combos_of(z, "weighted")[-1]
    order = orders(S, keep)
    r = np.array([o[len(o) // 3] for o in order])                # a listed news per user
    rs = torch.stack([S[u, r[u]] for u in range(U)])
    excl_id = np.array([next(int(x) for x in z["hist"][u].tolist() if 0 <= x < N and x != r[u]) for u in range(U)])
    inel_id = int(np.flatnonzero(~z["ok"].numpy())[3])
    out_id = int(np.flatnonzero(~keep.any(axis=0))[-1])
    variants = {"excluded": excl_id, "ineligible": np.full(U, inel_id), "outside": np.full(U, out_id), "negative": np.full(U, -5),
                "int32 min": np.full(U, -2 ** 31), "N": np.full(U, N), "past N": np.full(U, N + 3), "int32 max": np.full(U, BIG)}
    for what, ids in variants.items():
        for u in range(U):
            assert not keep[u, ids[u]] if 0 <= ids[u] < N else True
        cur = (rs.clone(), torch.from_numpy(ids.astype(np.int64)))
        for k in (5, 100):
            got = corpus.rank_topk(z["m"], z["p"], z["t"], k, **kw, **cursor_kw(cur))
            check_a(got, S, keep, cur, k, (what, k))
            first = got[1][:, 0].cpu().numpy()
            assert ((first == r) == (ids < r)).all(), what
    # a score no news has, between two listed ones, and ids of any kind
    mid = torch.stack([(S[u, order[u][10]] + S[u, order[u][11]]) / 2 for u in range(U)])
    cur = (mid, torch.from_numpy(excl_id.astype(np.int64)))
    check_a(corpus.rank_topk(z["m"], z["p"], z["t"], 20, **kw, **cursor_kw(cur)), S, keep, cur, 20, "between")


def test_sentinels_and_nan_per_user():
    """start, end and NaN cursors mixed over the users of one call (both users of a tile differ)."""
    z = world("small_f32", "weighted")
    U, N, S = z["U"], z["N"], z["S"]
    assert U == 5
    keep = base.keep_mask(U, N, z["hist"].numpy())
    kw = dict(exclude_ids=z["hist"].to(DEV))
    cs = torch.tensor([INF, -INF, NAN, INF, NAN])
    ci = torch.tensor([-1, BIG, -1, -1, BIG])
    for cs_, ci_ in ((cs, ci), (cs.flip(0), ci.flip(0))):
        cur = (cs_, ci_)
        for k in (10, 256):
            got = corpus.rank_topk(z["m"], z["p"], z["t"], k, **kw, **cursor_kw(cur))
            check_a(got, S, keep, cur, k, k)
            plain = corpus.rank_topk(z["m"], z["p"], z["t"], k, **kw)
            gi = got[1].cpu()
            for u in range(U):
                if cs_[u] == INF:
                    assert torch.equal(gi[u], plain[1][u].cpu()) and torch.equal(bits(got[0][u]), bits(plain[0][u]))
                else:
                    assert (gi[u] == -1).all() and torch.isneginf(got[0][u]).all()
    # the end sentinel's neighbours: (-inf, 2^31 - 2) still lists nothing here (no news scores -inf);
    # (-inf, -1), the tail of a short row, is not the end of the order in general (test_infinite_priors)
    cur = (torch.full((U,), -INF), torch.full((U,), BIG - 1))
    assert (corpus.rank_topk(z["m"], z["p"], z["t"], 10, **cursor_kw(cur))[1] == -1).all()


@pytest.mark.parametrize("shape", ["small_f32", "mid_f16"])
def test_infinite_priors(shape, monkeypatch):
    """+inf and -inf priors on several news: the pages walk through each group by id; a full row whose
    last entry is a -inf one continues with the rest of that group; a cursor at the (-inf, -1) tail
    would list the -inf news again, which is why page_cursor does not return it."""
    z = world(shape, "weighted")
    U, N = z["U"], z["N"]
    top = [5, 17, N // 2 + 2, N - 2]
    bottom = [0, 9, 33, N // 2 + 1, N - 1]
    bias = z["bias"][0].clone()
    bias[top], bias[bottom] = INF, -INF
    Sb = z["S"] + bias[None, :]
    keep = base.keep_mask(U, N)
    kw = dict(news_bias=bias.to(DEV))
    order = orders(Sb, keep)
    assert all(o[:4].tolist() == top and o[-5:].tolist() == bottom for o in order)
    # k = 3 ends inside the +inf group; kf: a whole number of full pages ends inside the -inf group
    kf = {200: 99, 1000: 249}[N]
    full_pages = N // kf
    j = full_pages * kf - 1 - (N - 5)                              # the last full page ends at bottom[j]
    assert 0 <= j < 4
    for split in ("0", "1"):
        monkeypatch.setenv("MINER_RK_SPLIT", split)
        for k in (3, kf, 256):
            npages = -(-N // k) + 2
            got = chain(z["m"], z["p"], z["t"], k, npages, kw)
            same(got, lists_after(Sb, keep, None, npages * k, order), (split, k))
    pages = chain(z["m"], z["p"], z["t"], kf, full_pages, kw)
    assert torch.isneginf(pages[0][:, -1]).all() and (pages[1][:, -1] == bottom[j]).all()     # full, and ends at -inf
    cs, ci = corpus.page_cursor((pages[0][:, -kf:], pages[1][:, -kf:]))
    assert torch.isneginf(cs).all() and ci.tolist() == [bottom[j]] * U
    rest = corpus.rank_topk(z["m"], z["p"], z["t"], kf, **kw, after=(cs, ci))
    assert rest[1][:, :5 - j].tolist() == [bottom[j + 1:] + [-1]] * U
    assert corpus.page_cursor(rest)[1].tolist() == [BIG] * U     # short: the end sentinel
    tail = (torch.full((U,), -INF), torch.full((U,), -1))
    again = corpus.rank_topk(z["m"], z["p"], z["t"], 10, **kw, **cursor_kw(tail))
    check_a(again, Sb, keep, tail, 10, "tail")
    assert again[1][:, :5].tolist() == [bottom] * U


@pytest.mark.parametrize("score_type", ["weighted", "max", "mean"])
def test_zero_scores_and_negative_zero(score_type):
    """Two all-zero table rows score exactly 0 in every score type; a cursor score of -0.0 is +0.0."""
    z = world("small_f32", score_type)
    U, N = z["U"], z["N"]
    a, b = 21, 150
    t = z["t"].clone()
    t[a], t[b] = 0, 0
    S = base.gpu_score_matrix(z["m"], z["p"], t, score_type)
    assert (S[:, a] == 0).all() and (S[:, b] == 0).all()
    keep = base.keep_mask(U, N)
    res = {}
    for zero in (0.0, -0.0):
        for n in (a, b, -1, BIG):
            cur = (torch.full((U,), zero), torch.full((U,), n))
            assert bool(torch.signbit(cur[0]).all()) == (str(zero) == "-0.0")
            got = corpus.rank_topk(z["m"], z["p"], t, 20, score_type=score_type, **cursor_kw(cur))
            check_a(got, S, keep, cur, 20, (zero, n))
            res[(str(zero), n)] = got
    for n in (a, b, -1, BIG):
        p0, n0 = res[("0.0", n)], res[("-0.0", n)]
        assert torch.equal(p0[1], n0[1]) and torch.equal(bits(p0[0]), bits(n0[0]))
    assert res[("-0.0", -1)][1][:, :2].tolist() == [[a, b]] * U
    assert (res[("-0.0", a)][1][:, 0] == b).all()
    assert not (res[("-0.0", b)][1] == b).any() and not (res[("-0.0", b)][1] == a).any()


@pytest.mark.parametrize("shape,score_type", [("small_f32", "weighted"), ("mid_f16", "weighted"), ("c5_bf16", "weighted"),
                                              ("small_f32", "max")])
def test_against_the_counting_form(shape, score_type):
    """For a page taken after a listed news c: rank_of(page ids)[j] == rank_of(c) + 1 + j — rank_of
    is the counting form, separately tested — without filters, with them, and under a prior."""
    z = world(shape, score_type)
    U, N = z["U"], z["N"]
    st = dict(score_type=score_type)
    forms = [dict(**st), dict(exclude_ids=z["hist"].to(DEV), eligible=z["ok"].to(DEV), **st),
             dict(exclude_ids=z["hist"].to(DEV), eligible=z["ok"].to(DEV), **biased.prior_kw(z), **st)]
    for kw in forms:
        first = corpus.rank_topk(z["m"], z["p"], z["t"], 40, **kw)
        for j0 in (0, 7, 39):
            c_s, c_i = first[0][:, j0].contiguous(), first[1][:, j0].contiguous()
            page = corpus.rank_topk(z["m"], z["p"], z["t"], 50, after=(c_s, c_i), **kw)
            assert (page[1] >= 0).all()
            rc = corpus.rank_of(z["m"], z["p"], z["t"], c_i[:, None], **kw)[0].cpu()
            rp, sp = corpus.rank_of(z["m"], z["p"], z["t"], page[1], **kw)
            assert (rc[:, 0] == j0).all()
            assert torch.equal(rp.cpu(), (rc + 1 + torch.arange(50)[None, :]).int()), j0
            assert torch.equal(bits(sp), bits(page[0]))


def depth_cursors(S, order, gen):
    """A different depth per user, from the start sentinel to the end sentinel: user u's cursor is the
    entry at a random position of its order (users 0 / 1: the sentinels; user 2: its last entry)."""
    U = S.shape[0]
    cs, ci = torch.empty(U), torch.empty(U, dtype=torch.int64)
    for u in range(U):
        o = order[u]
        j = int(torch.randint(0, len(o), (1,), generator=gen))
        if u == 2:
            j = len(o) - 1
        cs[u], ci[u] = S[u, o[j]], int(o[j])
    cs[0], ci[0] = INF, -1
    if U > 1:
        cs[1], ci[1] = -INF, BIG
    return cs, ci


@pytest.mark.parametrize("U", [515, 5])
def test_tiles_and_workgroups(U, monkeypatch):
    """U = 515: 258 two-user tiles over at most 256 workgroups (a workgroup's second tile takes its own
    users' cursors); U = 5: a tile with a user past U. Every user at its own depth."""
    K, d, N = 32, 64, 300
    m, p, t, gen = base.random_users(U + N + 2, U, K, d, N, torch.float32, dup=DUP)
    S = base.gpu_score_matrix(m, p, t, "weighted")
    excl = torch.randint(-1, N, (U, 30), generator=gen)
    ok = torch.rand(N, generator=gen) < 0.7
    sub, inside = biased.subset_ids(gen, N)
    bias = biased.make_prior(gen, N)
    group = torch.arange(U) % biased.G
    forms = [(dict(), S, base.keep_mask(U, N)),
             (dict(exclude_ids=excl.to(DEV), eligible=ok.to(DEV)), S, base.keep_mask(U, N, excl.numpy(), ok.numpy())),
             (dict(news_ids=sub.to(DEV)), S, base.keep_mask(U, N) & inside[None, :]),
             (dict(news_bias=bias.to(DEV), user_group=group.to(DEV)), S + bias[group], base.keep_mask(U, N))]
    for split in (("0", "1") if U == 5 else ("0",)):
        monkeypatch.setenv("MINER_RK_SPLIT", split)
        for kw, Sx, keep in forms:
            order = orders(Sx, keep)
            cur = depth_cursors(Sx, order, gen)
            for k in (10, 100):
                got = corpus.rank_topk(m, p, t, k, **kw, **cursor_kw(cur, torch.int32))
                same(got, lists_after(Sx, keep, cur, k, order), (U, split, sorted(kw), k))


def test_one_chunk_per_step():
    """fp16 at d = 64: a step is one chunk, so the epilogue — and the cursor test in it — sits between
    two consecutive chunk barriers."""
    U, K, d, N = 5, 32, 64, 600
    m, p, t, gen = base.random_users(66, U, K, d, N, torch.float16, dup=DUP)
    sub, inside = biased.subset_ids(gen, N)
    bias = biased.make_prior(gen, N)
    group = torch.arange(U) % biased.G
    for st in ("weighted", "mean"):
        S = base.gpu_score_matrix(m, p, t, st)
        forms = [(dict(), S, base.keep_mask(U, N)),
                 (dict(news_ids=sub.to(DEV)), S, base.keep_mask(U, N) & inside[None, :]),
                 (dict(news_bias=bias.to(DEV), user_group=group.to(DEV)), S + bias[group], base.keep_mask(U, N))]
        for kw, Sx, keep in forms:
            order = orders(Sx, keep)
            cur = depth_cursors(Sx, order, gen)
            for k in (10, 256):
                got = corpus.rank_topk(m, p, t, k, score_type=st, **kw, **cursor_kw(cur))
                same(got, lists_after(Sx, keep, cur, k, order), (st, sorted(kw), k))
            npages = -(-N // 100) + 2
            same(chain(m, p, t, 100, npages, dict(score_type=st, **kw)), lists_after(Sx, keep, None, npages * 100, order),
                 (st, sorted(kw), "chain"))


def test_rank_topk_deep():
    """N = 1000: topk = 600 (two full pages and a partial one) and 1200 (the tail), with exclusions
    and a prior, equal to yardstick A; topk = 100 is rank_topk bit for bit; after= continues."""
    z = world("mid_f16", "weighted")
    U, N = z["U"], z["N"]
    assert N == 1000
    pb = z["bias"][z["group"]].double().numpy()
    forms = [(dict(), z["S"], None, base.keep_mask(U, N)),
             (dict(exclude_ids=z["hist"].to(DEV), **biased.prior_kw(z)), z["Sb"], pb, base.keep_mask(U, N, z["hist"].numpy())),
             (dict(exclude_ids=z["hist"].to(DEV), eligible=z["ok"].to(DEV), news_ids=biased.subset_ids(torch.Generator().manual_seed(4), N)[0].to(DEV),
                   **biased.prior_kw(z)), z["Sb"], pb, None)]
    inside = biased.subset_ids(torch.Generator().manual_seed(4), N)[1]
    forms[2] = forms[2][:3] + (base.keep_mask(U, N, z["hist"].numpy(), z["ok"].numpy()) & inside[None, :],)
    for kw, S, prior, keep in forms:
        for topk in (600, 1200, 257, 1):
            got = corpus.rank_topk_deep(z["m"], z["p"], z["t"], topk, **kw)
            assert got[0].shape == (U, topk)
            check_a(got, S, keep, None, topk, (sorted(kw), topk))
            if topk == 1200:
                assert (got[1][:, -1] == -1).all()
                check_b(got, z["ref"], z["tol"], sorted(kw), prior)
        want = corpus.rank_topk(z["m"], z["p"], z["t"], 100, **kw)
        got = corpus.rank_topk_deep(z["m"], z["p"], z["t"], 100, **kw)
        assert torch.equal(got[1], want[1]) and torch.equal(bits(got[0]), bits(want[0]))
        # a given cursor continues from there: the deep list after the first 100 is entries 100..
        rest = corpus.rank_topk_deep(z["m"], z["p"], z["t"], 700, after=corpus.page_cursor(want), **kw)
        full = lists_after(S, keep, None, 800)
        same(rest, (full[0][:, 100:], full[1][:, 100:]), (sorted(kw), "after"))
        cur = (want[0][:, 49].cpu(), want[1][:, 49].cpu())
        check_a(corpus.rank_topk_deep(z["m"], z["p"], z["t"], 300, **kw, **cursor_kw(cur)), S, keep, cur, 300, "after 50")


def test_rank_corpus():
    """Two batch sizes give identical pages, equal to rank_topk on encode_users' output."""
    gen = torch.Generator().manual_seed(23)
    U, L, K, d, Dc, N = 5, 40, 32, 64, 96, 300
    table = (torch.randn(N, d, generator=gen) / d ** 0.5).to(DEV)
    mask = (torch.arange(L)[None, :] >= torch.randint(0, L - 4, (U, 1), generator=gen)).to(DEV)
    hid = torch.randint(0, N, (U, L), generator=gen).int().to(DEV)
    pk = corpus.pack_encoder((torch.randn(Dc, d, generator=gen) / d ** 0.5).to(DEV), (torch.randn(K, Dc, generator=gen) * 0.3).to(DEV),
                             (torch.randn(d, d, generator=gen) / d ** 0.5).to(DEV), dtype=torch.float32)
    mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
    seen = torch.where(mask, hid, -1)
    S = base.gpu_score_matrix(mui, proj, table, "weighted")
    keep = base.keep_mask(U, N, seen.cpu().numpy())
    order = orders(S, keep)
    cur = depth_cursors(S, order, gen)
    for after in (cursor_kw(cur)["after"], cursor_kw(cur, torch.int32)["after"], corpus.start_cursor(U, DEV)):
        a = corpus.rank_corpus(table, hid, mask, pk, 50, batch=2, exclude_history=True, after=after)
        b = corpus.rank_corpus(table, hid, mask, pk, 50, batch=U + 3, exclude_history=True, after=after)
        assert torch.equal(a[1], b[1]) and torch.equal(bits(a[0]), bits(b[0]))
        c = corpus.rank_topk(mui, proj, table, 50, exclude_ids=seen, after=after)
        assert torch.equal(a[1], c[1]) and torch.equal(bits(a[0]), bits(c[0]))
        same(a, lists_after(S, keep, (after[0].cpu(), after[1].cpu()), 50, order), "rank_corpus")
    page1 = corpus.rank_corpus(table, hid, mask, pk, 50, batch=2, exclude_history=True)
    page2 = corpus.rank_corpus(table, hid, mask, pk, 50, batch=3, exclude_history=True, after=corpus.page_cursor(page1))
    full = lists_after(S, keep, None, 100, order)
    same((torch.cat([page1[0], page2[0]], 1), torch.cat([page1[1], page2[1]], 1)), full, "two pages")


@pytest.mark.parametrize("shape,score_type", [("small_f32", "weighted"), ("mid_f16", "weighted"), ("c5_f16", "weighted"),
                                              ("small_f32", "mean")])
def test_no_cursor(shape, score_type, monkeypatch):
    """after=None, and start_cursor on every user: the lists of the plain call, bit for bit, in every form."""
    z = world(shape, score_type)
    U = z["U"]
    for split in ("0", "1"):
        monkeypatch.setenv("MINER_RK_SPLIT", split)
        for name, kw, S, prior, keep in combos_of(z, score_type):
            for topk in (10, 256):
                want = corpus.rank_topk(z["m"], z["p"], z["t"], topk, **kw)
                check_a(want, S, keep, None, topk, (name, topk))
                for after in (None, corpus.start_cursor(U, DEV)):
                    got = corpus.rank_topk(z["m"], z["p"], z["t"], topk, after=after, **kw)
                    assert torch.equal(got[1], want[1]) and torch.equal(bits(got[0]), bits(want[0])), (name, topk, split)
