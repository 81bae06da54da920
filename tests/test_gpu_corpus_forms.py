"""The ranker's C entry points are one function (include/miner_corpus.h: a wider entry with its
extra arguments NULL launches the narrower one's kernel) — needs an MI355X.

Direct ctypes calls, compared bit for bit with each other and with corpus.rank_topk, which always
calls the widest entry. What the lists must BE is the business of tests/test_gpu_corpus*.py; here
only that the chain of wrappers and the form table lose nothing on the way. U = 5 leaves a tile
with a user past U, K = 40 gives two interest tiles (K = 8 one), N = 300 one full and one partial
news step.
"""
import functools

import pytest
import torch

from miner_amd import _lib, corpus

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = {"k40_f16": (5, 40, 128, 300, 7, torch.float16), "k8_f32": (5, 8, 64, 300, 7, torch.float32)}
RANK = ("miner_rank_topk", "miner_rank_topk_ws", "miner_rank_topk_filtered", "miner_rank_topk_subset",
        "miner_rank_topk_biased", "miner_rank_topk_capped", "miner_rank_topk_after")


def bits(x):
    return x.view(torch.int32)


def ptr(x):
    return None if x is None else x.data_ptr()


@functools.lru_cache(maxsize=None)
def world(shape):
    U, K, d, N, topk, dtype = SHAPES[shape]
    gen = torch.Generator().manual_seed(K + d)
    m, p, t = (torch.randn(n, generator=gen).mul(0.3).to(DEV, dtype) for n in ((U, K, d), (U, K, d), (N, d)))
    excl = torch.randint(-1, N, (U, 9), generator=gen).int().to(DEV)          # -1: excludes nothing
    ok = corpus.pack_eligible((torch.rand(N, generator=gen) < 0.7).to(DEV))
    return dict(m=m, p=p, t=t, excl=excl, ok=ok, all_ids=torch.arange(N, dtype=torch.int32, device=DEV))


def rank(name, shape, excl=None, ok=None):
    """One miner_rank_topk* entry: the filters where it has them, nothing else optional."""
    U, K, d, N, topk, dtype = SHAPES[shape]
    z = world(shape)
    s = torch.empty(U, topk, dtype=torch.float32, device=DEV)
    i = torch.empty(U, topk, dtype=torch.int32, device=DEV)
    head = (torch.cuda.current_stream().cuda_stream, corpus._DT[dtype], _lib.SCORE_WEIGHTED, ptr(z["m"]), ptr(z["p"]),
            ptr(z["t"]), U, N, d, K, topk)
    flt = (ptr(excl), 0 if excl is None else excl.shape[1], ptr(ok))
    out = (ptr(s), ptr(i), None, 0)
    args = {"miner_rank_topk": head + out[:2],
            "miner_rank_topk_ws": head + out,
            "miner_rank_topk_filtered": head + flt + out,
            # the subset entry has no "whole table": every row, in the table's order
            "miner_rank_topk_subset": head + flt + (ptr(z["all_ids"]), N) + out,
            "miner_rank_topk_biased": head + flt + (None, -1) + out + (None, 0, None),
            "miner_rank_topk_capped": head + flt + (None, -1) + out + (None, 0, None, None, 0),
            "miner_rank_topk_after": head + flt + (None, -1) + out + (None, 0, None, None, 0, None, None)}[name]
    assert getattr(_lib.lib(), name)(*args) == 0, name
    return s, i


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rank_entries_without_options(shape):
    want = rank(RANK[0], shape)
    assert (want[1] >= 0).all() and torch.isfinite(want[0]).all()
    for name in RANK[1:]:
        assert same(rank(name, shape), want), name


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rank_entries_filtered(shape):
    z = world(shape)
    want = rank(RANK[2], shape, z["excl"], z["ok"])
    assert not same(want, rank(RANK[2], shape))               # the filters are no no-op
    for name in RANK[3:]:
        assert same(rank(name, shape, z["excl"], z["ok"]), want), name


@pytest.mark.parametrize("shape", list(SHAPES))
def test_pairs_count_merge(shape):
    U, K, d, N, topk, dtype = SHAPES[shape]
    z = world(shape)
    lib = _lib.lib()
    head = (torch.cuda.current_stream().cuda_stream, corpus._DT[dtype], _lib.SCORE_WEIGHTED, ptr(z["m"]), ptr(z["p"]),
            ptr(z["t"]), U, N, d, K)
    C = 11
    cand = torch.randint(-1, N + 1, (U, C), generator=torch.Generator().manual_seed(3)).int().to(DEV)
    sc = [torch.empty(U, C, dtype=torch.float32, device=DEV) for _ in range(2)]
    assert lib.miner_score_pairs(*head, ptr(cand), C, ptr(sc[0])) == 0
    assert lib.miner_score_pairs_biased(*head, ptr(cand), C, ptr(sc[1]), None, 0, None) == 0
    assert torch.equal(bits(sc[0]), bits(sc[1]))
    T = 3
    tid, tgt = cand[:, :T].contiguous(), sc[0][:, :T].contiguous()     # any (score, id) is a position in the order
    cnt = [torch.empty(U, T, dtype=torch.int32, device=DEV) for _ in range(2)]
    assert lib.miner_rank_count(*head, ptr(tgt), ptr(tid), T, ptr(z["ok"]), ptr(cnt[0])) == 0
    assert lib.miner_rank_count_biased(*head, ptr(tgt), ptr(tid), T, ptr(z["ok"]), ptr(cnt[1]), None, 0, None) == 0
    assert torch.equal(cnt[0], cnt[1]) and (cnt[0] >= 0).all() and (cnt[0] <= N).all()
    a, b = rank(RANK[0], shape), rank(RANK[2], shape, z["excl"], z["ok"])
    mg = [(torch.empty(U, topk, dtype=torch.float32, device=DEV), torch.empty(U, topk, dtype=torch.int32, device=DEV))
          for _ in range(2)]
    lists = (torch.cuda.current_stream().cuda_stream, ptr(a[0]), ptr(a[1]), topk, ptr(b[0]), ptr(b[1]), topk, U, topk,
             ptr(z["ok"]), N)
    assert lib.miner_topk_merge(*lists, ptr(mg[0][0]), ptr(mg[0][1])) == 0
    assert lib.miner_topk_merge_capped(*lists, ptr(mg[1][0]), ptr(mg[1][1]), None, 0, 0) == 0
    assert same(mg[0], mg[1]) and (mg[0][1] >= 0).any()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_python_calls_the_same_function(shape, monkeypatch):
    U, K, d, N, topk, dtype = SHAPES[shape]
    z = world(shape)
    for split in ("0", "1"):                                   # corpus.rank_topk with and without a workspace
        monkeypatch.setenv("MINER_RK_SPLIT", split)
        assert same(corpus.rank_topk(z["m"], z["p"], z["t"], topk), rank(RANK[-1], shape)), split
        got = corpus.rank_topk(z["m"], z["p"], z["t"], topk, exclude_ids=z["excl"], eligible=z["ok"])
        assert same(got, rank(RANK[-1], shape, z["excl"], z["ok"])), split
