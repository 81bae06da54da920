"""The ranker's filters (miner_rank_topk_filtered: per-user exclusion lists and the eligibility
bitmap; corpus.rank_topk / rank_corpus exclude_ids, exclude_history, eligible) — needs an MI355X.

* the filters only choose which (score, id) pairs are kept: at N <= 256 a filtered list equals the
  unfiltered one with the filtered ids struck out, bit for bit, then the (-inf, -1) tail;
* against the reference's own scores (tests/golden/corpus_c5_*.npz) and the oracle
  (oracle.corpus_oracle.corpus_scores) with the filtered entries set to -inf, at the bars of
  tests/test_gpu_corpus.py (fp32 1e-5·|ref| + 1e-5·rms, 16-bit ranker 2e-4 / 2e-4);
* partial bitmap words and news steps, fewer survivors than topk (and none), workgroups that walk
  several user tiles, split == unsplit, E = 0 / 1 / 256, batch independence, argument errors.
"""
import os

import numpy as np
import pytest
import torch

from miner_amd import corpus
from oracle import corpus_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
F32_TOL = dict(rtol=1e-5, rms_floor=1e-5)          # the bars of tests/test_gpu_corpus.py
RANK16_TOL = dict(rtol=2e-4, rms_floor=2e-4)


def load_corpus(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["score_type"] = str(g["score_type"])
    return g


def keep_mask(U, N, excl=None, ok=None):
    """bool [U,N]: the (user, news) pairs the filters let through. excl: integer [U,E] (entries
    outside [0, N) exclude nothing) or None; ok: bool [N] or None."""
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
    """check_topk of tests/test_gpu_corpus.py with the filtered entries of ref_scores [U,N] (float64)
    at -inf: n_ok = min(k, survivors), every returned id a survivor."""
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


def strike(full_s, full_i, keep, k):
    """The unfiltered complete list (every news of the table, best first) with the filtered ids
    struck out, cut / padded to k: what a filter that never touches a score must return."""
    fs, fi = full_s.cpu(), full_i.cpu()
    U = fi.shape[0]
    es = torch.full((U, k), float("-inf"))
    ei = torch.full((U, k), -1, dtype=torch.int32)
    for u in range(U):
        valid = fi[u] >= 0
        sel = valid.clone()
        sel[valid] = torch.from_numpy(keep[u])[fi[u][valid].long()]
        n = min(k, int(sel.sum()))
        es[u, :n] = fs[u][sel][:n]
        ei[u, :n] = fi[u][sel][:n]
    return es, ei


def random_users(seed, U, K, d, N, dtype):
    gen = torch.Generator().manual_seed(seed)
    mui = torch.randn(U, K, d, generator=gen) / 2
    proj = torch.randn(U, K, d, generator=gen) / 2
    table = torch.randn(N, d, generator=gen) / d ** 0.5
    m, p, t = (x.to(DEV, dtype) for x in (mui, proj, table))
    return m, p, t, gen


def oracle_scores(m, p, t, score_type="weighted"):
    return co.corpus_scores(m.float().cpu(), p.float().cpu(), t.float().cpu(), score_type).double().numpy()


@pytest.fixture(scope="module")
def small():
    """U = 5, L = 40, K = 32, d = 64, Dc = 96, N = 200, fp32: encoded users, their histories (with
    padded slots), a 50 % bitmap and per score type the complete unfiltered list (topk = 256)."""
    gen = torch.Generator().manual_seed(21)
    U, L, K, d, Dc, N = 5, 40, 32, 64, 96, 200
    table = torch.randn(N, d, generator=gen) / d ** 0.5
    hl = torch.randint(5, L + 1, (U,), generator=gen)
    mask = torch.arange(L)[None, :] >= (L - hl)[:, None]
    hid = torch.randint(0, N, (U, L), generator=gen)
    W1 = torch.randn(Dc, d, generator=gen) / d ** 0.5
    Q = torch.randn(K, Dc, generator=gen) * 0.3
    W2 = torch.randn(d, d, generator=gen) / d ** 0.5
    ok = torch.rand(N, generator=gen) < 0.5
    pk = corpus.pack_encoder(W1.to(DEV), Q.to(DEV), W2.to(DEV), dtype=torch.float32)
    tab = table.to(DEV)
    mui, proj = corpus.encode_users(tab, mask.to(DEV), pk, his_ids=hid.to(DEV).int())
    full = {st: tuple(x.clone() for x in corpus.rank_topk(mui, proj, tab, 256, score_type=st))
            for st in ("weighted", "max", "mean")}
    for s, i in full.values():
        assert (i[:, :N] >= 0).all() and (i[:, N:] == -1).all()
    seen = torch.where(mask, hid, torch.full_like(hid, -1))
    return dict(U=U, N=N, tab=tab, mui=mui, proj=proj, pk=pk, hid=hid, mask=mask, seen=seen, ok=ok, full=full)


@pytest.mark.parametrize("score_type", ["weighted", "max", "mean"])
def test_filters_only_strike_entries(small, score_type):
    """N <= 256: history exclusion, a 50 % bitmap and both against the complete list, bitwise."""
    z = small
    fs, fi = z["full"][score_type]
    cases = {"history": (z["seen"], None), "bitmap": (None, z["ok"]), "both": (z["seen"], z["ok"])}
    for name, (excl, ok) in cases.items():
        ts, ti = corpus.rank_topk(z["mui"], z["proj"], z["tab"], 256, score_type=score_type,
                                  exclude_ids=None if excl is None else excl.to(DEV),
                                  eligible=None if ok is None else ok.to(DEV))
        keep = keep_mask(z["U"], z["N"], None if excl is None else excl.numpy(), None if ok is None else ok.numpy())
        assert not keep.all()
        es, ei = strike(fs, fi, keep, 256)
        assert torch.equal(ti.cpu(), ei), (score_type, name)
        assert torch.equal(ts.cpu(), es), (score_type, name)


@pytest.mark.parametrize("name", ["corpus_c5_weighted", "corpus_c5_max"])
def test_exclude_history_matches_reference(name):
    """rank_corpus(exclude_history=True) against the reference's own scores with every user's
    clicked news at -inf (more rows than the largest topk survive for every user: no tail)."""
    g = load_corpus(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    table, hid, mask = t(g["table"]), t(g["his_ids"]), t(g["his_mask"])
    w2 = t(g["W2"]) if "W2" in g else None
    pk = corpus.pack_encoder(t(g["W1"]), t(g["Q"]), w2, dtype=torch.float32)
    ref = g["scores"].astype(np.float64)
    U, N = ref.shape
    keep = keep_mask(U, N, np.where(g["his_mask"].astype(bool), g["his_ids"], -1))
    assert (keep.sum(1) >= 256).all() and not keep.all()       # 522 of 700 / 431 of 600 at the least
    for k in (17, 256):
        ts, ti = corpus.rank_corpus(table, hid, mask, pk, k, score_type=g["score_type"], exclude_history=True)
        check_filtered(ts, ti, ref, keep, k, F32_TOL)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_partial_words_and_steps(dtype):
    """N = 1000 (three full 256-steps + 232 rows; the last bitmap word has 8 valid bits, its unused
    high bits set), U = 3 (the last tile holds one user), d = 128, K = 64."""
    U, K, d, N = 3, 64, 128, 1000
    m, p, t, gen = random_users(31, U, K, d, N, dtype)
    tol = F32_TOL if dtype == torch.float32 else RANK16_TOL
    ref = oracle_scores(m, p, t)
    ok = torch.rand(N, generator=gen) < 0.5
    ok[N - 1] = True
    words = corpus.pack_eligible(ok.to(DEV))
    assert words.shape == ((N + 31) // 32,) and words.dtype == torch.int32
    words[-1] |= -256                                           # bits 8..31 of the last word: news >= N
    real = torch.stack([torch.from_numpy(np.argsort(-ref[u])[:12].copy()) for u in range(U)])   # the users' best
    junk = torch.tensor([[-1, N, N + 23, 2 ** 31 - 1, -7]] * U)
    a = corpus.rank_topk(m, p, t, 100, exclude_ids=real.to(DEV), eligible=words)
    b = corpus.rank_topk(m, p, t, 100, exclude_ids=torch.cat([junk[:, :2], real, junk[:, 2:]], 1).to(DEV), eligible=words)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "ids outside [0, N) changed the list"
    check_filtered(a[0], a[1], ref, keep_mask(U, N, real.numpy(), ok.numpy()), 100, tol)
    # the table's last news, in the last valid bit: with fewer survivors than topk every survivor is returned
    sparse = torch.rand(N, generator=gen) < 0.15
    sparse[N - 1] = True
    w2 = corpus.pack_eligible(sparse.to(DEV))
    w2[-1] |= -256
    ts, ti = corpus.rank_topk(m, p, t, 256, eligible=w2)
    assert int(sparse.sum()) < 256
    check_filtered(ts, ti, ref, keep_mask(U, N, None, sparse.numpy()), 256, tol)
    assert ((ti == N - 1).sum(1) == 1).all()
    assert (ti < N).all()


@pytest.mark.parametrize("split", ["0", "1"])
def test_fewer_survivors_than_topk(split, monkeypatch):
    """N = 300, topk = 100: 37 eligible news -> 37 entries and the tail; no eligible news, or a user
    whose exclusion list holds every eligible id -> that row all (-inf, -1)."""
    monkeypatch.setenv("MINER_RK_SPLIT", split)
    U, K, d, N, k = 5, 32, 64, 300, 100
    m, p, t, gen = random_users(41, U, K, d, N, torch.float32)
    ref = oracle_scores(m, p, t)
    ok = torch.zeros(N, dtype=torch.bool)
    ok[torch.randperm(N, generator=gen)[:37]] = True
    ts, ti = corpus.rank_topk(m, p, t, k, eligible=ok.to(DEV))
    check_filtered(ts, ti, ref, keep_mask(U, N, None, ok.numpy()), k, F32_TOL)
    assert ((ti >= 0).sum(1) == 37).all()
    ts, ti = corpus.rank_topk(m, p, t, k, eligible=torch.zeros(N, dtype=torch.bool, device=DEV))
    assert (ti == -1).all() and torch.isneginf(ts).all()
    excl = torch.full((U, 37), -1, dtype=torch.long)
    excl[2] = torch.nonzero(ok)[:, 0]
    ts, ti = corpus.rank_topk(m, p, t, k, exclude_ids=excl.to(DEV), eligible=ok.to(DEV))
    check_filtered(ts, ti, ref, keep_mask(U, N, excl.numpy(), ok.numpy()), k, F32_TOL)
    assert (ti[2] == -1).all() and torch.isneginf(ts[2]).all() and ((ti >= 0).sum(1).cpu() == torch.tensor([37, 37, 0, 37, 37])).all()


@pytest.mark.parametrize("split,U,N", [("1", 70, 600), ("0", 515, 300)])
def test_several_tiles_per_workgroup(split, U, N, monkeypatch):
    """More user tiles than workgroups take them in one pass (split: 35 tiles over 32 tile slots;
    unsplit: 258 tiles over 256 workgroups): each tile must rank under its own users' lists. Every
    user excludes its own best 24 news, so another tile's list leaves them in."""
    monkeypatch.setenv("MINER_RK_SPLIT", split)
    K, d, k = 32, 64, 20
    m, p, t, gen = random_users(U + N, U, K, d, N, torch.float32)
    ref = oracle_scores(m, p, t)
    excl = np.argsort(-ref, axis=1)[:, :24].copy()
    ts, ti = corpus.rank_topk(m, p, t, k, exclude_ids=torch.from_numpy(excl).to(DEV))
    check_filtered(ts, ti, ref, keep_mask(U, N, excl), k, F32_TOL)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("U,N,topk", [(37, 5000, 7), (3, 200, 256)])
def test_split_equals_unsplit_filtered(dtype, U, N, topk, monkeypatch):
    """The split form filters inside the per-slice ranker; its merged list is the unsplit one's, bit
    for bit (duplicated news rows force exact score ties across slices)."""
    gen = torch.Generator().manual_seed(U + N)
    K, d = 64, 768
    table = torch.randn(N, d, generator=gen) / d ** 0.5
    table[N // 2:N // 2 + 50] = table[:50]
    mui = (torch.randn(U, K, d, generator=gen) / 4).to(DEV, dtype)
    proj = (torch.randn(U, K, d, generator=gen) / 4).to(DEV, dtype)
    tab = table.to(DEV, dtype)
    excl = torch.randint(-1, N, (U, 50), generator=gen).to(DEV)
    ok = corpus.pack_eligible((torch.rand(N, generator=gen) < 0.5).to(DEV))
    for st in ("weighted", "max"):
        monkeypatch.setenv("MINER_RK_SPLIT", "1")
        a = corpus.rank_topk(mui, proj, tab, topk, score_type=st, exclude_ids=excl, eligible=ok)
        monkeypatch.setenv("MINER_RK_SPLIT", "0")
        b = corpus.rank_topk(mui, proj, tab, topk, score_type=st, exclude_ids=excl, eligible=ok)
        c = corpus.rank_topk(mui, proj, tab, topk, score_type=st)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), st
        assert not torch.equal(b[1], c[1]), "the filters changed nothing"


def test_exclusion_width_edges(small):
    """E = 0 is no exclusion; E = 1; E = 256 (the cap) with duplicates — against the complete list."""
    z = small
    U, N = z["U"], z["N"]
    fs, fi = z["full"]["weighted"]
    gen = torch.Generator().manual_seed(7)
    ts, ti = corpus.rank_topk(z["mui"], z["proj"], z["tab"], 256, exclude_ids=torch.empty(U, 0, dtype=torch.int64, device=DEV))
    assert torch.equal(ts, fs) and torch.equal(ti, fi)
    one = fi[:, :1].cpu().long()                               # every user's best news
    wide = torch.randint(0, 60, (U, 256), generator=gen)       # 256 draws of 60 ids: duplicates
    wide[:, 255] = one[:, 0]                                   # the last slot counts
    for excl in (one, wide):
        ts, ti = corpus.rank_topk(z["mui"], z["proj"], z["tab"], 256, exclude_ids=excl.to(DEV))
        es, ei = strike(fs, fi, keep_mask(U, N, excl.numpy()), 256)
        assert torch.equal(ti.cpu(), ei) and torch.equal(ts.cpu(), es), excl.shape
        assert (ti[:, 0].cpu() != one[:, 0]).all()


def test_rank_corpus_batches_with_exclude_history(small):
    """Each user's filtered list is independent of the batching: the lists are sliced with the
    histories. With extra exclude_ids and a bitmap on top."""
    z = small
    hid, mask, tab = z["hid"].to(DEV).int(), z["mask"].to(DEV), z["tab"]
    a = corpus.rank_corpus(tab, hid, mask, z["pk"], 30, exclude_history=True, batch=2)
    b = corpus.rank_corpus(tab, hid, mask, z["pk"], 30, exclude_history=True, batch=z["U"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    es, ei = strike(*z["full"]["weighted"], keep_mask(z["U"], z["N"], z["seen"].numpy()), 30)
    assert torch.equal(b[1].cpu(), ei) and torch.equal(b[0].cpu(), es)
    extra = z["full"]["weighted"][1][:, :3].long()
    a = corpus.rank_corpus(tab, hid, mask, z["pk"], 30, exclude_history=True, exclude_ids=extra,
                           eligible=z["ok"].to(DEV), batch=2)
    b = corpus.rank_corpus(tab, hid, mask, z["pk"], 30, exclude_history=True, exclude_ids=extra,
                           eligible=corpus.pack_eligible(z["ok"].to(DEV)), batch=z["U"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    both = torch.cat([z["seen"], extra.cpu()], 1).numpy()
    es, ei = strike(*z["full"]["weighted"], keep_mask(z["U"], z["N"], both, z["ok"].numpy()), 30)
    assert torch.equal(b[1].cpu(), ei) and torch.equal(b[0].cpu(), es)


def test_filter_argument_errors(small):
    z = small
    U, N = z["U"], z["N"]
    mui, proj, tab = z["mui"], z["proj"], z["tab"]
    zi = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        corpus.rank_topk(mui, proj, tab, 5, exclude_ids=zi(U, 257))
    with pytest.raises(ValueError):
        corpus.rank_topk(mui, proj, tab, 5, exclude_ids=zi(U + 1, 4))
    with pytest.raises(ValueError):
        corpus.rank_topk(mui, proj, tab, 5, eligible=zi((N + 31) // 32 + 1))
    with pytest.raises(ValueError):
        corpus.rank_topk(mui, proj, tab, 5, eligible=torch.ones(N + 1, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        corpus.rank_topk(mui, proj, tab, 5, eligible=torch.ones(N, device=DEV))
    with pytest.raises(ValueError):                       # history (40) + 217 extra ids
        corpus.rank_corpus(tab, z["hid"].to(DEV).int(), z["mask"].to(DEV), z["pk"], 5, exclude_history=True,
                           exclude_ids=zi(U, 217))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        corpus.rank_topk(mui, proj, tab, 5, exclude_ids=torch.zeros(U, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        corpus.rank_topk(mui, proj, tab, 5, eligible=torch.ones(N, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        corpus.pack_eligible(torch.ones(N, dtype=torch.bool))
