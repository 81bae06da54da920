"""The score-prior entry points on the host: miner_rank_topk_biased, miner_score_pairs_biased and
miner_rank_count_biased are exported and declared, the prior table's argument errors
(include/miner_corpus.h) are answered with their codes after the unbiased call's own checks and
before any launch — with U = 0 or C = 0 where the arguments are accepted, so nothing launches —,
and the ABI number is unchanged. The Python-side argument errors of news_bias= / user_group= are
raised before anything touches a device. The AddressSanitizer driver of the three entry points
(tests/native/abi_errors_bias.cpp) runs as tests/test_asan_abi.py runs the first one. No compute
call is made (runs on CPU-only machines)."""
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
NAMES = ("miner_rank_topk_biased", "miner_score_pairs_biased", "miner_rank_count_biased")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library()
    return _lib.lib()


def p(v):
    return None if v is None else P(v)


def topk(lib, *, bias=80, G=1, grp=None, ids=None, M=-1, excl=16, E=2, ok=48, U=0, N=100, K=32, d=64, k=10, mui=16,
         proj=16, news=16, dtype=F32, st=WEIGHTED, out_s=32, out_i=64, ws=None):
    return lib.miner_rank_topk_biased(None, dtype, st, p(mui), p(proj), p(news), U, N, d, K, k, p(excl), E, p(ok), p(ids), M,
                                      p(out_s), p(out_i), p(ws), 0, p(bias), G, p(grp))


def pairs(lib, *, bias=80, G=1, grp=None, ids=16, C=8, out=32, U=0, N=100, K=32, d=64, mui=16, proj=16, news=16,
          dtype=F32, st=WEIGHTED):
    return lib.miner_score_pairs_biased(None, dtype, st, p(mui), p(proj), p(news), U, N, d, K, p(ids), C, p(out), p(bias), G,
                                        p(grp))


def count(lib, *, bias=80, G=1, grp=None, ts=16, ti=32, T=4, ok=48, out=64, U=0, N=100, K=32, d=64, mui=16, proj=16,
          news=16, dtype=F32, st=WEIGHTED):
    return lib.miner_rank_count_biased(None, dtype, st, p(mui), p(proj), p(news), U, N, d, K, p(ts), p(ti), T, p(ok), p(out),
                                       p(bias), G, p(grp))


FORMS = (topk, pairs, count)


def test_symbols_are_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert ctypes.cast(getattr(raw, name), ctypes.c_void_p).value
    assert lib.miner_abi_version() == 6 == _lib.ABI_VERSION      # the entry points are additive
    # each is its unbiased form's signature plus (news_bias, G, user_group)
    tail = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    for name, base in zip(NAMES, ("miner_rank_topk_subset", "miner_score_pairs", "miner_rank_count")):
        assert _lib.SIGNATURES[name] == (ctypes.c_int, _lib.SIGNATURES[base][1] + tail)
    for name in ("rank_topk", "score_pairs", "rank_of", "update_topk", "rescore_topk", "rank_corpus", "evaluate_corpus"):
        params = inspect.signature(getattr(corpus, name)).parameters
        for kw in ("news_bias", "user_group"):
            assert params[kw].kind is inspect.Parameter.KEYWORD_ONLY and params[kw].default is None, (name, kw)


@pytest.mark.parametrize("form", FORMS)
def test_prior_argument_errors_in_order_before_any_launch(lib, form):
    for U in (0, 3):                                             # with users too: still no launch
        assert form(lib, U=U, G=0) == EINVAL                     # a table without rows
        assert form(lib, U=U, G=-4, grp=96) == EINVAL
        assert form(lib, U=U, bias=None, grp=96) == EINVAL       # groups without a table
        assert form(lib, U=U, bias=None, G=0, grp=96) == EINVAL
        assert form(lib, U=U, bias=82) == EALIGN                 # 4-byte alignment
        assert form(lib, U=U, grp=98, G=2) == EALIGN
        assert form(lib, U=U, bias=82, grp=98) == EALIGN
        assert form(lib, U=U, bias=82, G=0) == EINVAL            # G, then the alignment
        assert form(lib, U=U, bias=None, grp=98) == EINVAL       # a table for the groups, then the alignment
    # accepted argument sets: U = 0 returns after the validation, nothing launches
    assert form(lib) == OK
    assert form(lib, G=3, grp=96) == OK
    assert form(lib, bias=84, grp=100, G=2 ** 31 - 1) == OK      # 4-byte, not 16-byte, aligned
    assert form(lib, bias=None, G=0) == OK                       # no prior: the unbiased call
    assert form(lib, bias=None, G=5) == OK                       # G is read only with a table


def test_empty_work_returns_ok_without_a_launch(lib):
    assert pairs(lib, U=3, C=0) == OK                            # C == 0 with users
    assert pairs(lib, U=3, C=0, ids=None, out=None, G=2, grp=96) == OK
    assert pairs(lib, U=3, C=0, G=0) == EINVAL                   # ... after the prior's checks
    assert topk(lib, U=0, ids=None, M=0) == OK                   # an empty id list
    assert topk(lib, U=0, ids=16, M=0) == OK
    assert topk(lib, U=0, ids=16, M=5, G=3, grp=96) == OK        # the subset form
    assert count(lib, U=0, T=64, ok=None) == OK


def test_the_unbiased_checks_still_come_first(lib):
    bad = dict(bias=82, G=0, grp=98)                             # every prior argument invalid as well
    for form in FORMS:
        assert form(lib, dtype=9, **bad) == EINVAL
        assert form(lib, K=65, **bad) == ESHAPE
        assert form(lib, d=100, **bad) == ESHAPE
        assert form(lib, st=7, **bad) == EINVAL
        assert form(lib, U=-1, **bad) == EINVAL
        assert form(lib, N=0, **bad) == EINVAL
        assert form(lib, mui=None, **bad) == EINVAL
        assert form(lib, proj=None, **bad) == EINVAL             # weighted needs the projection
        assert form(lib, news=20, **bad) == EALIGN
    assert topk(lib, k=0, **bad) == EINVAL
    assert topk(lib, k=corpus.MAX_TOPK + 1, **bad) == ESHAPE
    assert topk(lib, E=-1, **bad) == EINVAL
    assert topk(lib, E=corpus.MAX_L + 1, **bad) == ESHAPE
    assert topk(lib, excl=18, **bad) == EALIGN
    assert topk(lib, ok=50, **bad) == EALIGN
    assert topk(lib, ids=16, M=-1, **bad) == EINVAL              # the subset rules: a list with M < 0
    assert topk(lib, ids=None, M=4, **bad) == EINVAL             # a length without a list
    assert topk(lib, ids=18, M=4, **bad) == EALIGN
    assert pairs(lib, C=-1, **bad) == EINVAL
    assert pairs(lib, ids=18, bias=82) == EALIGN
    assert pairs(lib, out=None, C=3, **bad) == EINVAL
    assert count(lib, T=0, **bad) == EINVAL
    assert count(lib, T=corpus.MAX_TARGETS + 1, **bad) == ESHAPE
    assert count(lib, out=66, **bad) == EALIGN


def test_python_argument_errors():
    U, K, d, N = 3, 4, 64, 50
    mui = torch.zeros(U, K, d)
    tab = torch.zeros(N, d)
    ids = torch.zeros(U, 5, dtype=torch.int64)
    lists = (torch.zeros(U, 5), ids)
    grp = torch.tensor([0, 1, 1])
    calls = {
        "rank_topk": lambda **kw: corpus.rank_topk(mui, mui, tab, 5, **kw),
        "score_pairs": lambda **kw: corpus.score_pairs(mui, mui, tab, ids, **kw),
        "rank_of": lambda **kw: corpus.rank_of(mui, mui, tab, ids, **kw),
        "update_topk": lambda **kw: corpus.update_topk(lists, mui, mui, tab, ids[0], **kw),
        "rescore_topk": lambda **kw: corpus.rescore_topk(lists, mui, mui, tab, **kw),
    }
    for name, call in calls.items():
        for bad in (torch.zeros(N + 1), torch.zeros(2, N + 1), torch.zeros(N, 2), torch.zeros(1, 1, N), torch.zeros(0, N),
                    torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float16),
                    torch.zeros(N, dtype=torch.int32), [0.0] * N):
            with pytest.raises(ValueError):
                call(news_bias=bad)
        with pytest.raises(ValueError):
            call(news_bias=torch.zeros(2, N))                     # [G, N] without user_group
        with pytest.raises(ValueError):
            call(user_group=grp)                                  # groups without a prior
        for bad in (grp[:2], grp[None, :], grp.float(), grp == 0):
            with pytest.raises(ValueError):
                call(news_bias=torch.zeros(2, N), user_group=bad)
        for bad in (torch.tensor([0, 2, 1]), torch.tensor([0, -1, 1])):
            with pytest.raises(ValueError):
                call(news_bias=torch.zeros(2, N), user_group=bad)     # a group out of range
        with pytest.raises(ValueError):
            call(news_bias=torch.zeros(N), user_group=grp)        # G = 1: group 1 is out of range
        # well-formed, but not on a GPU: no CPU path
        for kw in (dict(news_bias=torch.zeros(N)), dict(news_bias=torch.zeros(1, N)),
                   dict(news_bias=torch.zeros(2, N), user_group=grp)):
            with pytest.raises(RuntimeError):
                call(**kw)
    L = 6
    hid, mask = torch.zeros(U, L, dtype=torch.int32), torch.ones(U, L, dtype=torch.bool)
    pk = corpus.EncoderWeights(torch.zeros(16, dtype=torch.uint8), torch.float32, d, 8, K, True)
    for call in (lambda **kw: corpus.rank_corpus(tab, hid, mask, pk, 5, **kw),
                 lambda **kw: corpus.evaluate_corpus(tab, hid, mask, pk, ids, **kw)):
        with pytest.raises(ValueError):
            call(news_bias=torch.zeros(N - 1))
        with pytest.raises(ValueError):
            call(news_bias=torch.zeros(2, N))
        with pytest.raises(ValueError):
            call(news_bias=torch.zeros(2, N), user_group=torch.tensor([0, 1, 2]))
        with pytest.raises(ValueError):
            call(news_bias=torch.zeros(2, N), user_group=grp[:2])  # one group per user of the whole call
        with pytest.raises(RuntimeError):
            call(news_bias=torch.zeros(2, N), user_group=grp)


@pytest.fixture(scope="module")
def driver():
    try:
        return build.build_asan_driver(driver="bias")
    except RuntimeError as e:                       # no ROCm toolchain in this environment
        pytest.skip(f"asan build unavailable: {e}")


def test_new_entry_points_under_asan(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    res = subprocess.run([driver], capture_output=True, text=True, timeout=300, env=env)
    out = res.stdout + res.stderr
    assert "AddressSanitizer" not in out, out[-4000:]
    assert res.returncode == 0, out[-4000:]
    assert "0 failures" in res.stdout, out[-2000:]
