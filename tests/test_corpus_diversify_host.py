"""The diversity re-ranking on the host (include/miner_diversify.h, corpus.diversify_topk /
rank_topk_diverse): the float64 verifier of tests/diversify_ref.py has the power it is used for (it
accepts the definition's own output and rejects the undiversified order and a single swapped pair),
miner_topk_diversify is exported and declared, its argument errors come back with their codes in the
documented order and before any launch (host pointers through ctypes, U = 0 where the arguments are
accepted), the Python-side errors are raised before anything touches a device, and the
AddressSanitizer driver tests/native/abi_errors_diversify.cpp (a stand-alone program) reports
nothing. No compute call is made (runs on CPU-only machines).

``random_inputs`` is shared with tests/test_gpu_corpus_diversify.py."""
import ctypes
import functools
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import diversify_ref as ref
from miner_amd import _lib, build, corpus

OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3
F32, BF16, F16 = _lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16
REL_SCORE, REL_MINMAX = 0, 1
P = ctypes.c_void_p
N_TABLE = 512


@functools.lru_cache(maxsize=None)
def random_inputs(seed, dtype, d, pool, U, N=N_TABLE):
    """(scores [U,pool] fp32, ids [U,pool] int64, table [N,d] dtype) on the CPU. Table rows: a third
    normal, a third heavy-tailed (Student t, 2 degrees of freedom, clipped to ±100), a third
    near-copies of the first third (the row plus a tenth of its scale in noise), so that a pool
    holds both near-duplicates and unrelated rows. Scores normal, ids distinct per user."""
    g = np.random.default_rng(seed)
    third = N // 3
    tab = np.empty((N, d))
    tab[:third] = g.standard_normal((third, d))
    tab[third:2 * third] = np.clip(g.standard_t(2, (third, d)), -100, 100)
    tab[2 * third:] = tab[:N - 2 * third] + 0.1 * g.standard_normal((N - 2 * third, d))
    table = torch.from_numpy(tab).to(dtype)
    scores = torch.from_numpy(g.standard_normal((U, pool)).astype(np.float32))
    ids = torch.from_numpy(np.stack([g.permutation(N)[:pool] for _ in range(U)]))
    return scores, ids, table


# ---- the power of the verifier ----------------------------------------------------------------------
POWER = [(torch.float16, 64, 100), (torch.float32, 768, 100), (torch.bfloat16, 64, 256)]


def relevance_order(scores, ids, N, topk):
    """The undiversified list: the candidates by score, ties by position."""
    s = scores.numpy().astype(np.float64)
    out = []
    for u in range(s.shape[0]):
        cand = np.flatnonzero((ids[u].numpy() >= 0) & (ids[u].numpy() < N) & np.isfinite(s[u]))
        pos = cand[np.lexsort((cand, -s[u, cand]))][:topk]
        out.append(np.concatenate([pos, np.full(topk - len(pos), -1)]))
    return np.stack(out)


def as_got(pos, scores, ids):
    """(out_scores, out_ids, out_pos) of the list that holds the pool's positions ``pos`` (-1: tail)."""
    pos = np.asarray(pos)
    safe = np.clip(pos, 0, None)
    s = np.where(pos >= 0, np.take_along_axis(scores.numpy(), safe, 1), -np.inf).astype(np.float32)
    i = np.where(pos >= 0, np.take_along_axis(ids.numpy(), safe, 1), -1)
    return s, i, pos


@pytest.mark.parametrize("dtype,d,pool", POWER)
@pytest.mark.parametrize("relevance", ["minmax", "score"])
def test_check_accepts_the_definition(dtype, d, pool, relevance):
    scores, ids, table = random_inputs(11, dtype, d, pool, 5)
    for topk in (10, pool):
        got = ref.greedy(scores, ids, table, topk, 0.5, relevance)
        assert ref.check(got, (scores, ids, table, topk, 0.5, relevance), dtype) == 0.0
        ref.check(got[:3], (scores, ids, table, topk, 0.5, relevance), dtype)      # without out_obj


@pytest.mark.parametrize("dtype,d,pool", POWER)
def test_check_rejects_the_undiversified_order_and_a_swapped_pair(dtype, d, pool):
    scores, ids, table = random_inputs(11, dtype, d, pool, 5)
    lam, topk = 0.5, pool
    inputs = (scores, ids, table, topk, lam, "minmax")
    with pytest.raises(AssertionError, match="step"):
        ref.check(as_got(relevance_order(scores, ids, table.shape[0], topk), scores, ids), inputs, dtype)
    # two adjacent picks swapped at a step whose objective gap exceeds 10 tol_obj
    _, _, pos, obj = ref.greedy(scores, ids, table, topk, lam, "minmax")
    tab64 = ref._np(table)
    swapped = 0
    for u in range(scores.shape[0]):
        cand, rel, sim = ref._user(scores[u].numpy(), ids[u].numpy(), tab64, lam, "minmax")
        _, tol_obj = ref.tolerances(d, lam, float(np.abs(rel[cand]).max()))
        m = np.zeros(pool)
        for t in range(topk - 1):
            p, q = int(pos[u, t]), int(pos[u, t + 1])
            gap = obj[u, t] - (lam * rel[q] - (1 - lam) * m[q])      # the next pick's objective at step t
            if gap > 10 * tol_obj:
                bad = pos.copy()
                bad[u, t], bad[u, t + 1] = q, p
                with pytest.raises(AssertionError, match=f"user {u}.*step {t}:"):
                    ref.check(as_got(bad, scores, ids), inputs, dtype)
                swapped += 1
                break
            m = sim[:, p].copy() if t == 0 else np.maximum(m, sim[:, p])
    assert swapped == scores.shape[0], "the seed must give every user a step with a gap above 10 tol_obj"
    # ... and a broken bookkeeping field each: score bits, ids, a repeated position, a short row
    got = [a.copy() for a in ref.greedy(scores, ids, table, topk, lam, "minmax")]
    for k, (field, value) in enumerate([(0, np.float32(0.125)), (1, -5), (2, got[2][0, 0]), (2, -1)]):
        bad = [a.copy() for a in got]
        bad[field][0, 1 if k == 2 else 3] = value
        with pytest.raises(AssertionError):
            ref.check(bad, inputs, dtype)


# ---- the C ABI -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library()
    return _lib.lib()


def p(v):
    return None if v is None else P(v)


def call(lib, *, dtype=F16, news=16, N=1000, d=768, in_s=256, in_i=512, U=0, pool=256, k=100, lam=0.7, rel=REL_MINMAX,
         out_s=1024, out_i=2048, out_p=3072, out_o=3584):
    return lib.miner_topk_diversify(None, dtype, p(news), N, d, p(in_s), p(in_i), U, pool, k, lam, rel, p(out_s), p(out_i),
                                    p(out_p), p(out_o))


def test_symbol_is_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert "miner_topk_diversify" in _lib.SIGNATURES
    assert ctypes.cast(raw.miner_topk_diversify, ctypes.c_void_p).value
    assert lib.miner_abi_version() == 6 == _lib.ABI_VERSION       # the entry point is additive
    I, V = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["miner_topk_diversify"] == (I, [V, I, V, I, I, V, V, I, I, I, ctypes.c_float, I, V, V, V, V])
    assert os.path.join(build.HERE, "csrc", "diversify.hip") in build.SOURCES
    assert os.path.join(build.ROOT, "include", "miner_diversify.h") in build.HEADERS
    params = inspect.signature(corpus.diversify_topk).parameters
    assert list(params) == ["lists", "news", "topk", "lam", "relevance", "return_positions", "return_objective"]
    assert params["topk"].default is None and params["lam"].default == 0.7 and params["relevance"].default == "minmax"
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(params)[3:])
    params = inspect.signature(corpus.rank_topk_diverse).parameters
    assert list(params) == ["user_mui", "user_proj", "news", "topk", "pool", "lam", "relevance", "rank_kwargs"]
    assert params["pool"].default is None and params["rank_kwargs"].kind is inspect.Parameter.VAR_KEYWORD


def test_argument_errors_in_order_before_any_launch(lib):
    for U in (0, 3):                                              # with users too: still no launch
        # 1. dtype, relevance
        for bad in (9, -1, _lib.DTYPE_F32_MFMA, _lib.DTYPE_F32_X6):
            assert call(lib, U=U, dtype=bad) == EINVAL
        for bad in (2, -1, 77):
            assert call(lib, U=U, rel=bad) == EINVAL
        # 2. sizes
        assert call(lib, U=U, N=0) == EINVAL
        assert call(lib, U=U, N=-4) == EINVAL
        assert call(lib, U=U, pool=0, k=0) == EINVAL
        assert call(lib, U=U, pool=-1) == EINVAL
        assert call(lib, U=U, k=0) == EINVAL
        assert call(lib, U=U, k=-7) == EINVAL
        # 3. required pointers
        for name in ("news", "in_s", "in_i", "out_s", "out_i", "out_p"):
            assert call(lib, U=U, **{name: None}) == EINVAL, name
        # 4. lambda
        for bad in (-0.001, 1.001, float("nan"), float("inf"), float("-inf")):
            assert call(lib, U=U, lam=bad) == EINVAL, bad
        # 5. shapes
        assert call(lib, U=U, pool=257) == ESHAPE
        assert call(lib, U=U, pool=100, k=101) == ESHAPE
        for dtype, bad in ((F16, 0), (F16, -64), (F16, 96), (F16, 32), (BF16, 32), (F32, 48), (F32, 16), (F16, 1088),
                           (F32, 1056)):
            assert call(lib, U=U, dtype=dtype, d=bad) == ESHAPE, (dtype, bad)
        # 6. alignment
        assert call(lib, U=U, news=20) == EALIGN                  # 4-byte, not 16-byte
        for name in ("in_s", "in_i", "out_s", "out_i", "out_p", "out_o"):
            assert call(lib, U=U, **{name: 1026}) == EALIGN, name
        # the order: every class with the later ones wrong as well
        later = dict(news=20, in_s=258)
        assert call(lib, U=U, d=100, pool=300, k=400, **later) == ESHAPE
        assert call(lib, U=U, lam=2.0, d=100, pool=300, k=400, **later) == EINVAL
        assert call(lib, U=U, out_p=None, lam=2.0, d=100, pool=300, **later) == EINVAL
        assert call(lib, U=U, rel=5, N=0, in_i=None, lam=-1.0, d=100, **later) == EINVAL
        assert call(lib, U=U, pool=257, news=20) == ESHAPE
    assert call(lib, U=-1) == EINVAL
    assert call(lib, U=0, news=20) == EALIGN                      # before the U == 0 return
    # accepted argument sets: U = 0 returns after the validation, nothing launches
    assert call(lib) == OK
    assert call(lib, out_o=None) == OK                            # out_obj is optional
    assert call(lib, in_s=260, in_i=516, out_s=1028, out_i=2052, out_p=3076, out_o=3588) == OK   # 4-byte aligned
    for lam in (0.0, 1.0, 0.3):
        assert call(lib, lam=lam) == OK
    assert call(lib, rel=REL_SCORE, pool=1, k=1) == OK
    assert call(lib, pool=256, k=256) == OK
    assert call(lib, dtype=F32, d=32) == OK
    assert call(lib, dtype=BF16, d=1024, N=2 ** 31 - 1) == OK


# ---- Python --------------------------------------------------------------------------------------------
def test_python_argument_errors():
    U, K, d, N, k = 3, 4, 64, 50, 8
    s, i = torch.zeros(U, k), torch.zeros(U, k, dtype=torch.int64)
    g = torch.zeros(U, k, dtype=torch.int32)
    tab = torch.zeros(N, d)
    div = corpus.diversify_topk
    for lists in ((s,), (s, i.float()), (s, i[:, :4]), (s, i, g[:, :4]), (s, i, g.float()), (s, i, None), (s, i, g, g), s,
                  (s[0], i[0]), (s, i[:2], g)):
        with pytest.raises(ValueError):                           # neither a pair nor a triple
            div(lists, tab)
    with pytest.raises(ValueError, match="more than 256"):
        div((torch.zeros(U, 257), torch.zeros(U, 257, dtype=torch.int32)), tab)
    with pytest.raises(ValueError):
        div((s[:, :0], i[:, :0]), tab)
    for bad in (k + 1, 0, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="topk"):
            div((s, i), tab, bad)
    for bad in (-0.1, 1.0001, float("nan"), "0.5", None, True, torch.tensor(0.5)):
        with pytest.raises(ValueError, match="lam"):
            div((s, i), tab, lam=bad)
    for bad in ("rank", "MINMAX", None, 1):
        with pytest.raises(ValueError, match="relevance"):
            div((s, i), tab, relevance=bad)
    for bad in (torch.zeros(N, 48), torch.zeros(N, 1088), torch.zeros(N, 32, dtype=torch.float16), torch.zeros(N),
                torch.zeros(0, d), torch.zeros(2, N, d)):
        with pytest.raises(ValueError):
            div((s, i), bad)
    with pytest.raises(TypeError):
        div((s, i), torch.zeros(N, d, dtype=torch.float64))
    # well-formed, but not on a GPU: no CPU path
    for kw in (dict(), dict(topk=1), dict(lam=0, relevance="score"), dict(lam=1, return_positions=True)):
        with pytest.raises(RuntimeError):
            div((s, i), tab, **kw)
    with pytest.raises(RuntimeError):
        div((s, i.to(torch.int16), g.long()), tab.half())
    with pytest.raises(RuntimeError):
        div((s, i), torch.zeros(N, 32))                           # fp32 takes d % 32 == 0

    mui = torch.zeros(U, K, d)
    rtd = functools.partial(corpus.rank_topk_diverse, mui, mui, tab)
    with pytest.raises(ValueError, match="pool"):
        rtd(10, pool=9)
    with pytest.raises(ValueError, match="pool"):
        rtd(10, pool=257)
    with pytest.raises(ValueError, match="pool"):
        rtd(10, pool=20.0)
    with pytest.raises(ValueError, match="resume"):
        rtd(10, resume=corpus.start_walk(U, "cpu"), news_cluster=torch.zeros(N, dtype=torch.int64), cluster_cap=1)
    for bad in (0, 257, 2.0, True):
        with pytest.raises(ValueError, match="topk"):
            rtd(bad)
    with pytest.raises(ValueError, match="lam"):
        rtd(10, lam=1.5)
    with pytest.raises(ValueError, match="relevance"):
        rtd(10, relevance="zscore")
    with pytest.raises(ValueError):
        rtd(10, news_cluster=torch.zeros(N, dtype=torch.int64))   # rank_topk's own checks pass through
    with pytest.raises(TypeError):
        rtd(10, no_such_argument=1)
    with pytest.raises(RuntimeError):
        rtd(10)                                                   # well-formed, not on a GPU
    with pytest.raises(RuntimeError):
        rtd(10, pool=10, resume=None)


# ---- the host code under AddressSanitizer (a stand-alone program) ------------------------------------
def test_the_driver_is_found_by_its_name():
    assert build.asan_drivers()["diversify"] == os.path.join(build.ASAN_DRIVER_DIR, "abi_errors_diversify.cpp")


@pytest.fixture(scope="module")
def driver():
    try:
        return build.build_asan_driver(driver="diversify")
    except RuntimeError as e:                       # no ROCm toolchain in this environment
        pytest.skip(f"asan build unavailable: {e}")


def test_new_entry_point_under_asan(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1")
    res = subprocess.run([driver], capture_output=True, text=True, timeout=300, env=env)
    out = res.stdout + res.stderr
    assert "AddressSanitizer" not in out, out[-4000:]
    assert res.returncode == 0, out[-4000:]
    assert "0 failures" in res.stdout, out[-2000:]
