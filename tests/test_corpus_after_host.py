"""Keyset cursors on the host: miner_rank_topk_after is exported and declared as
miner_rank_topk_capped plus two pointers, the cursor's argument errors (include/miner_corpus.h) are
answered with their codes after the capped call's own checks and before any launch — with U = 0
where the arguments are accepted, so nothing launches —, and the ABI number is unchanged. The
Python-side argument errors of after= are raised before anything touches a device, and
start_cursor / page_cursor are checked on CPU tensors against hand-written rows. The
AddressSanitizer driver of the entry point (tests/native/abi_errors_after.cpp, a stand-alone
program) runs as tests/test_corpus_cap_host.py runs its own. No compute call is made (runs on
CPU-only machines)."""
import ctypes
import inspect
import os
import subprocess

import pytest
import torch

from miner_amd import _lib, build, corpus

OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3
F32, WEIGHTED = _lib.DTYPE_F32, _lib.SCORE_WEIGHTED
P = ctypes.c_void_p
INF = float("inf")
BIG = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library()
    return _lib.lib()


def p(v):
    return None if v is None else P(v)


def after(lib, *, aft_s=144, aft_i=160, clus=None, cap=0, bias=None, G=0, grp=None, ids=None, M=-1, excl=16, E=2, ok=48,
          U=0, N=100, K=32, d=64, k=10, mui=16, proj=16, news=16, dtype=F32, st=WEIGHTED, out_s=32, out_i=64, ws=None):
    return lib.miner_rank_topk_after(None, dtype, st, p(mui), p(proj), p(news), U, N, d, K, k, p(excl), E, p(ok), p(ids), M,
                                     p(out_s), p(out_i), p(ws), 0, p(bias), G, p(grp), p(clus), cap, p(aft_s), p(aft_i))


def test_symbol_and_signatures(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert "miner_rank_topk_after" in _lib.SIGNATURES
    assert ctypes.cast(raw.miner_rank_topk_after, ctypes.c_void_p).value
    assert lib.miner_abi_version() == 6 == _lib.ABI_VERSION      # the entry point is additive
    I, V = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["miner_rank_topk_after"] == (I, _lib.SIGNATURES["miner_rank_topk_capped"][1] + [V, V])
    for name in ("rank_topk", "rank_corpus", "rank_topk_deep"):
        params = inspect.signature(getattr(corpus, name)).parameters
        assert params["after"].kind is inspect.Parameter.KEYWORD_ONLY and params["after"].default is None, name
    assert list(inspect.signature(corpus.start_cursor).parameters) == ["U", "device"]
    assert list(inspect.signature(corpus.page_cursor).parameters) == ["lists"]
    deep = inspect.signature(corpus.rank_topk_deep).parameters
    assert list(deep)[:4] == ["user_mui", "user_proj", "news", "topk"]
    for kw in ("score_type", "exclude_ids", "eligible", "news_ids", "news_bias", "user_group"):
        assert deep[kw].kind is inspect.Parameter.KEYWORD_ONLY and deep[kw].default == inspect.signature(corpus.rank_topk).parameters[kw].default
    # unchanged: no cursor there
    for name in ("update_topk", "rescore_topk", "merge_topk", "rank_of", "score_pairs", "evaluate_corpus", "cap_topk"):
        assert "after" not in inspect.signature(getattr(corpus, name)).parameters, name


def test_cursor_argument_errors_in_order_before_any_launch(lib):
    for U in (0, 3):                                             # with users too: still no launch
        assert after(lib, U=U, aft_i=None) == EINVAL             # one word without the other
        assert after(lib, U=U, aft_s=None) == EINVAL
        assert after(lib, U=U, aft_s=146, aft_i=None) == EINVAL  # the pair, then the alignment
        assert after(lib, U=U, clus=112, cap=2) == EINVAL        # a cursor together with a cluster table
        assert after(lib, U=U, clus=112, cap=2, aft_s=146, aft_i=162) == EINVAL   # ... then the alignment
        assert after(lib, U=U, aft_s=146) == EALIGN              # 4-byte alignment
        assert after(lib, U=U, aft_i=162) == EALIGN
        assert after(lib, U=U, aft_s=145, aft_i=161, bias=80, G=3, grp=96, ids=16, M=5) == EALIGN
    # accepted argument sets: U = 0 returns after the validation, nothing launches
    assert after(lib) == OK
    assert after(lib, aft_s=148, aft_i=164) == OK                # 4-byte, not 16-byte, aligned
    assert after(lib, excl=None, E=0, ok=None) == OK             # no filter
    assert after(lib, bias=80, G=3, grp=96) == OK                # with a prior
    assert after(lib, ids=16, M=5) == OK                         # the subset form
    assert after(lib, ids=16, M=0) == OK
    assert after(lib, ws=256) == OK                              # a workspace is accepted
    assert after(lib, cap=-9) == OK                              # cap is read only with a table


def test_both_null_is_the_capped_call(lib):
    none = dict(aft_s=None, aft_i=None)
    assert after(lib, **none) == OK
    assert after(lib, clus=112, cap=2, **none) == OK             # caps without a cursor: the capped call's answer
    assert after(lib, clus=116, cap=corpus.MAX_TOPK, bias=80, G=3, grp=96, ids=16, M=5, **none) == OK
    assert after(lib, clus=112, cap=0, **none) == EINVAL
    assert after(lib, clus=112, cap=corpus.MAX_TOPK + 1, **none) == ESHAPE
    assert after(lib, clus=114, cap=2, **none) == EALIGN
    cap_sig = _lib.SIGNATURES["miner_rank_topk_capped"][1]
    args = [None, F32, WEIGHTED, P(16), P(16), P(16), 0, 100, 64, 32, 10, P(16), 2, P(48), None, -1, P(32), P(64), None, 0,
            None, 0, None, P(112), 2]
    assert len(args) == len(cap_sig)
    assert lib.miner_rank_topk_capped(*args) == lib.miner_rank_topk_after(*args, None, None) == OK


def test_the_older_checks_still_come_first(lib):
    bad = dict(aft_s=146, aft_i=None)                            # the cursor invalid as well
    assert after(lib, dtype=9, **bad) == EINVAL
    assert after(lib, K=65, **bad) == ESHAPE
    assert after(lib, d=100, **bad) == ESHAPE
    assert after(lib, st=7, **bad) == EINVAL
    assert after(lib, U=-1, **bad) == EINVAL
    assert after(lib, N=0, **bad) == EINVAL
    assert after(lib, mui=None, **bad) == EINVAL
    assert after(lib, proj=None, **bad) == EINVAL                # weighted needs the projection
    assert after(lib, news=20, aft_s=144, aft_i=None) == EALIGN
    assert after(lib, k=0, aft_s=146, aft_i=160) == EINVAL
    assert after(lib, k=corpus.MAX_TOPK + 1, **bad) == ESHAPE
    assert after(lib, E=corpus.MAX_L + 1, **bad) == ESHAPE
    assert after(lib, excl=18, aft_s=144, aft_i=None) == EALIGN
    assert after(lib, ok=50, aft_s=144, aft_i=None) == EALIGN
    assert after(lib, ids=18, M=4, aft_s=144, aft_i=None) == EALIGN          # the subset rules
    assert after(lib, ids=None, M=4, aft_s=146, aft_i=160) == EINVAL
    assert after(lib, bias=82, G=1, aft_s=144, aft_i=None) == EALIGN         # the prior's checks
    assert after(lib, bias=80, G=0, aft_s=146, aft_i=160) == EINVAL
    assert after(lib, clus=112, cap=corpus.MAX_TOPK + 1, **bad) == ESHAPE    # the caps' checks
    assert after(lib, clus=114, cap=2, aft_s=144, aft_i=None) == EALIGN


def test_python_argument_errors():
    U, K, d, N = 3, 4, 64, 50
    mui = torch.zeros(U, K, d)
    tab = torch.zeros(N, d)
    L = 6
    hid, mask = torch.zeros(U, L, dtype=torch.int32), torch.ones(U, L, dtype=torch.bool)
    pk = corpus.EncoderWeights(torch.zeros(16, dtype=torch.uint8), torch.float32, d, 8, K, True)
    calls = {
        "rank_topk": lambda **kw: corpus.rank_topk(mui, mui, tab, 5, **kw),
        "rank_topk_deep": lambda **kw: corpus.rank_topk_deep(mui, mui, tab, 300, **kw),
        "rank_corpus": lambda **kw: corpus.rank_corpus(tab, hid, mask, pk, 5, **kw),
    }
    s, i = torch.zeros(U), torch.zeros(U, dtype=torch.int64)
    clus = torch.arange(N) % 4
    wrong = [s, (s,), (s, i, i), (s.double(), i), (s.half(), i), (s[:2], i), (s, i[:2]), (s[None, :], i), (s, i[:, None]),
             (s, i.float()), (s, i == 0), ([0.0] * U, i), (s, [0] * U), (torch.zeros(U + 1), torch.zeros(U + 1, dtype=torch.int64)),
             (s, torch.tensor([0, 2 ** 31, 0])), (s, torch.tensor([0, -2 ** 31 - 1, 0]))]      # ids past int32
    for name, call in calls.items():
        for bad in wrong:
            with pytest.raises(ValueError):
                call(after=bad)
        # well-formed, but not on a GPU: no CPU path
        for good in ((s, i), (s, i.int()), (s, i.to(torch.int16)), (s, torch.tensor([BIG, -2 ** 31, 0])),
                     corpus.start_cursor(U, "cpu"), (torch.tensor([INF, -INF, float("nan")]), i)):
            with pytest.raises(RuntimeError):
                call(after=good)
    # no cursor under caps
    for name in ("rank_topk", "rank_corpus"):
        with pytest.raises(ValueError):
            calls[name](after=(s, i), news_cluster=clus, cluster_cap=2)
    for kw in (dict(news_cluster=clus, cluster_cap=2), dict(news_cluster=clus), dict(cluster_cap=1),
               dict(after=(s, i), news_cluster=clus, cluster_cap=2)):
        with pytest.raises(ValueError):
            calls["rank_topk_deep"](**kw)
    for bad in (0, -1, 2.0, "5", True, None):
        with pytest.raises(ValueError):
            corpus.rank_topk_deep(mui, mui, tab, bad)


def test_start_and_page_cursor_on_cpu_tensors():
    s, i = corpus.start_cursor(4, "cpu")
    assert s.dtype == torch.float32 and i.dtype == torch.int32 and s.shape == i.shape == (4,)
    assert (s == INF).all() and (i == -1).all()
    e = corpus.start_cursor(0, "cpu")
    assert e[0].shape == e[1].shape == (0,)
    scores = torch.tensor([[3.0, 2.0, 1.0],        # full
                           [3.0, 2.0, -INF],       # short: one tail entry
                           [-INF, -INF, -INF],     # empty
                           [0.5, -INF, -INF],      # full, its last entries real news that score -inf
                           [2.0, 2.0, -0.0]])      # full, a tie and a negative zero
    ids = torch.tensor([[7, 9, 4], [5, 0, -1], [-1, -1, -1], [8, 2, 6], [1, 3, 0]])
    for dt in (torch.int32, torch.int64):
        cs, ci = corpus.page_cursor((scores, ids.to(dt)))
        assert cs.dtype == torch.float32 and ci.dtype == torch.int32 and cs.shape == ci.shape == (5,)
        assert cs.is_contiguous() and ci.is_contiguous()
        assert ci.tolist() == [4, BIG, BIG, 6, 0]
        assert torch.equal(cs.view(torch.int32), torch.tensor([1.0, -INF, -INF, -INF, -0.0]).view(torch.int32))
    one = corpus.page_cursor((scores[:, :1], ids[:, :1]))         # k = 1
    assert one[1].tolist() == [7, 5, BIG, 8, 1] and one[0].tolist() == [3.0, 3.0, -INF, 0.5, 2.0]
    for bad in ((scores,), scores, (scores, ids[:, :2]), (scores[0], ids[0]), (scores, ids.float()), (scores[:, :0], ids[:, :0]),
                (ids, ids)):
        with pytest.raises(ValueError):
            corpus.page_cursor(bad)


@pytest.fixture(scope="module")
def driver():
    try:
        return build.build_asan_driver(driver="after")
    except RuntimeError as e:                       # no ROCm toolchain in this environment
        pytest.skip(f"asan build unavailable: {e}")


def test_new_entry_point_under_asan(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    res = subprocess.run([driver], capture_output=True, text=True, timeout=300, env=env)
    out = res.stdout + res.stderr
    assert "AddressSanitizer" not in out, out[-4000:]
    assert res.returncode == 0, out[-4000:]
    assert "0 failures" in res.stdout, out[-2000:]
