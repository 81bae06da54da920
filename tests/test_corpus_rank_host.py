"""miner_score_pairs and miner_rank_count on the host: both symbols are exported and declared, every
argument error the header documents (include/miner_corpus.h) is answered with its code before any
launch — with U = 0 or C = 0 where the arguments are accepted, so nothing launches —, the checks
shared with miner_rank_topk_filtered still come first, and the ABI number is unchanged. The
Python-side argument errors of score_pairs / rank_of / corpus_metrics are raised before anything
touches a device. The AddressSanitizer driver of the two entry points
(tests/native/abi_errors_rank.cpp) runs as tests/test_asan_abi.py runs the first one. No compute
call is made (runs on CPU-only machines)."""
import ctypes
import os
import subprocess

import pytest
import torch

from miner_amd import _lib, build, corpus

OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3
F32, WEIGHTED = _lib.DTYPE_F32, _lib.SCORE_WEIGHTED
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library()
    return _lib.lib()


def pairs(lib, *, ids=16, C=8, out=32, U=0, N=100, K=32, d=64, mui=16, proj=16, news=16, dtype=F32, st=WEIGHTED):
    p = lambda v: None if v is None else P(v)
    return lib.miner_score_pairs(None, dtype, st, p(mui), p(proj), p(news), U, N, d, K, p(ids), C, p(out))


def count(lib, *, ts=16, ti=32, T=4, ok=48, out=64, U=0, N=100, K=32, d=64, mui=16, proj=16, news=16, dtype=F32,
          st=WEIGHTED):
    p = lambda v: None if v is None else P(v)
    return lib.miner_rank_count(None, dtype, st, p(mui), p(proj), p(news), U, N, d, K, p(ts), p(ti), T, p(ok), p(out))


def test_symbols_are_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("miner_score_pairs", "miner_rank_count"):
        assert name in _lib.SIGNATURES
        assert ctypes.cast(getattr(raw, name), ctypes.c_void_p).value
    assert lib.miner_abi_version() == 6 == _lib.ABI_VERSION      # the entry points are additive
    assert corpus.MAX_TARGETS == 64
    for name in ("score_pairs", "rank_of", "corpus_metrics", "evaluate_corpus", "rescore_topk"):
        assert callable(getattr(corpus, name))


def test_score_pairs_argument_errors_before_any_launch(lib):
    assert pairs(lib, C=-1) == EINVAL
    assert pairs(lib, ids=None, C=3) == EINVAL                    # a length without a list
    assert pairs(lib, out=None, C=3) == EINVAL
    assert pairs(lib, ids=18) == EALIGN                           # 4-byte alignment
    assert pairs(lib, out=34) == EALIGN
    assert pairs(lib, ids=18, C=0) == EALIGN
    assert pairs(lib, U=3, C=-1) == EINVAL                        # the same with users: still no launch
    assert pairs(lib, U=3, ids=None, C=3) == EINVAL
    assert pairs(lib, U=3, out=34) == EALIGN
    # accepted argument sets: U = 0 or C = 0 returns after validation, nothing launches
    assert pairs(lib) == OK
    assert pairs(lib, U=3, C=0) == OK
    assert pairs(lib, U=3, ids=None, out=None, C=0) == OK
    assert pairs(lib, ids=20, out=36) == OK
    assert pairs(lib, st=_lib.SCORE_MAX, proj=None) == OK


def test_rank_count_argument_errors_before_any_launch(lib):
    assert count(lib, T=0) == EINVAL
    assert count(lib, T=-1) == EINVAL
    assert count(lib, ts=None) == EINVAL
    assert count(lib, ti=None) == EINVAL
    assert count(lib, out=None) == EINVAL
    assert count(lib, T=corpus.MAX_TARGETS + 1) == ESHAPE
    for name in ("ts", "ti", "ok", "out"):
        assert count(lib, **{name: 18}) == EALIGN, name
    assert count(lib, ts=None, T=corpus.MAX_TARGETS + 1) == EINVAL   # NULL, then the cap, then the alignment
    assert count(lib, ts=18, T=corpus.MAX_TARGETS + 1) == ESHAPE
    assert count(lib, U=3, T=0) == EINVAL                         # with users: still before any launch
    assert count(lib, U=3, T=65) == ESHAPE
    assert count(lib, U=3, ok=18) == EALIGN
    # accepted: U = 0 returns after validation; the bitmap may be NULL
    assert count(lib) == OK
    assert count(lib, T=1) == OK
    assert count(lib, T=corpus.MAX_TARGETS, ok=None) == OK
    assert count(lib, st=_lib.SCORE_MEAN, proj=None) == OK


def test_the_shared_checks_still_come_first(lib):
    # each with an invalid argument of the new function's own as well: the older check's code is returned
    for fn, bad in ((pairs, dict(ids=None, C=-5)), (count, dict(ts=None, T=-5))):
        assert fn(lib, dtype=9, **bad) == EINVAL
        assert fn(lib, K=65, **bad) == ESHAPE
        assert fn(lib, d=100, **bad) == ESHAPE
        assert fn(lib, st=7, **bad) == EINVAL
        assert fn(lib, U=-1, **bad) == EINVAL
        assert fn(lib, N=0, **bad) == EINVAL
        assert fn(lib, mui=None, **bad) == EINVAL
        assert fn(lib, news=None, **bad) == EINVAL
        assert fn(lib, proj=None, **bad) == EINVAL                # weighted needs the projection
        assert fn(lib, mui=20, **bad) == EALIGN
        assert fn(lib, news=20, **bad) == EALIGN
    assert pairs(lib, d=100, ids=18) == ESHAPE                    # the shape before the misaligned list
    assert count(lib, mui=20, T=65) == EALIGN                     # the user pointer before the target cap


def test_python_argument_errors():
    U, K, d, N = 3, 4, 64, 50
    mui = torch.zeros(U, K, d)
    tab = torch.zeros(N, d)
    ids = torch.zeros(U, 5, dtype=torch.int64)
    with pytest.raises(ValueError):
        corpus.rank_of(mui, mui, tab, torch.zeros(U, corpus.MAX_TARGETS + 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        corpus.rank_of(mui, mui, tab, torch.zeros(U, 0, dtype=torch.int32))
    with pytest.raises(ValueError):
        corpus.rank_of(mui, mui, tab, ids.float())                # float ids
    with pytest.raises(ValueError):
        corpus.rank_of(mui, mui, tab, ids[:2])                    # one row per user
    with pytest.raises(ValueError):
        corpus.rank_of(mui, mui, tab, ids[0])                     # [U, T]
    with pytest.raises(ValueError):
        corpus.rank_of(mui, mui, tab, ids, exclude_ids=torch.zeros(U, corpus.MAX_L + 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        corpus.rank_of(mui, mui, tab, ids, exclude_ids=ids.float())
    with pytest.raises(ValueError):
        corpus.score_pairs(mui, mui, tab, ids.float())
    with pytest.raises(ValueError):
        corpus.score_pairs(mui, mui, tab, ids == 0)               # bool ids
    with pytest.raises(ValueError):
        corpus.score_pairs(mui, mui, tab, ids[:, 0])
    with pytest.raises(ValueError):
        corpus.score_pairs(mui, mui, tab, ids[:1])
    with pytest.raises(ValueError):
        corpus.corpus_metrics(torch.zeros(U, 2))                  # ranks are integers
    with pytest.raises(RuntimeError):
        corpus.score_pairs(mui, mui, tab, ids)                    # well-formed, but not on a GPU: no CPU path


@pytest.fixture(scope="module")
def driver():
    try:
        return build.build_asan_driver(driver="rank")
    except RuntimeError as e:                       # no ROCm toolchain in this environment
        pytest.skip(f"asan build unavailable: {e}")


def test_new_entry_points_under_asan(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    res = subprocess.run([driver], capture_output=True, text=True, timeout=300, env=env)
    out = res.stdout + res.stderr
    assert "AddressSanitizer" not in out, out[-4000:]
    assert res.returncode == 0, out[-4000:]
    assert "0 failures" in res.stdout, out[-2000:]
