"""miner_rank_topk_filtered on the host: the symbol is exported, and every argument error the
filters add (include/miner_corpus.h) is answered with its documented code before any launch; the
eligibility bitmap's bit order through the packing expression of corpus.pack_eligible. No compute
call is made (runs on CPU-only machines)."""
import ctypes
import os

import pytest
import torch

from miner_amd import _lib, corpus

OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3
F32, WEIGHTED = _lib.DTYPE_F32, _lib.SCORE_WEIGHTED


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from miner_amd.build import build_library
        build_library()
    return _lib.lib()


def call(lib, *, excl=16, E=4, ok=16, U=3, topk=10, K=32, d=64, ws=None):
    P = ctypes.c_void_p
    return lib.miner_rank_topk_filtered(None, F32, WEIGHTED, P(16), P(16), P(16), U, 100, d, K, topk,
                                        None if excl is None else P(excl), E, None if ok is None else P(ok),
                                        P(16), P(16), None if ws is None else P(ws), 0)


def test_symbol_is_exported(lib):
    assert "miner_rank_topk_filtered" in _lib.SIGNATURES
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert ctypes.cast(raw.miner_rank_topk_filtered, ctypes.c_void_p).value
    assert lib.miner_abi_version() == 6 == _lib.ABI_VERSION


def test_filter_argument_errors_before_any_launch(lib):
    assert call(lib, E=-1) == EINVAL
    assert call(lib, excl=None, E=4) == EINVAL                  # a width without a list
    assert call(lib, E=corpus.MAX_L + 1) == ESHAPE
    assert call(lib, excl=18) == EALIGN                         # 4-byte alignment, both pointers
    assert call(lib, ok=17) == EALIGN
    assert call(lib, excl=18, E=0) == EALIGN
    # U = 0 returns after validation, before any launch: these argument sets are accepted
    assert call(lib, U=0) == OK
    assert call(lib, U=0, E=corpus.MAX_L) == OK
    assert call(lib, U=0, excl=None, E=0, ok=None) == OK
    assert call(lib, U=0, excl=20, E=0, ok=4) == OK             # E == 0 with any pointer; 4-byte aligned


def test_the_unfiltered_checks_still_come_first(lib):
    assert call(lib, topk=0) == EINVAL
    assert call(lib, topk=corpus.MAX_TOPK + 1) == ESHAPE
    assert call(lib, K=65) == ESHAPE
    assert call(lib, d=100) == ESHAPE
    assert lib.miner_rank_topk_ws(None, F32, WEIGHTED, ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16),
                                  0, 100, 64, 32, 10, ctypes.c_void_p(16), ctypes.c_void_p(16), None, 0) == OK


@pytest.mark.parametrize("N", [1, 31, 32, 33, 64, 1000])
def test_bit_order(N):
    """news n -> bit n & 31 (bit 0 least significant) of word n >> 5, for every single-news mask
    position that matters (word edges, the sign bit, the table's last news) and a random mask."""
    for n in sorted({0, min(N - 1, 1), min(N - 1, 31), min(N - 1, 32), N - 1}):
        mask = torch.zeros(N, dtype=torch.bool)
        mask[n] = True
        w = corpus._pack_bits(mask)
        assert w.dtype == torch.int32 and w.shape == ((N + 31) // 32,)
        want = [0] * ((N + 31) // 32)
        want[n >> 5] = 1 << (n & 31)
        assert [int(x) & 0xFFFFFFFF for x in w] == want, (N, n)
    gen = torch.Generator().manual_seed(N)
    mask = torch.rand(N, generator=gen) < 0.5
    w = [int(x) & 0xFFFFFFFF for x in corpus._pack_bits(mask)]
    for n in range(N):
        assert (w[n >> 5] >> (n & 31)) & 1 == int(mask[n])
    for n in range(N, 32 * len(w)):
        assert (w[n >> 5] >> (n & 31)) & 1 == 0                # bits past N are written as 0
