"""The dominant interest of a (user, news) pair, pinned on the CPU against the reference's own forward
pass (tests/golden/interest/corpus_interest_c5_*.npz, made by tests/golden/make_interest_golden.py).

This module holds the numpy restatement that tests/test_gpu_corpus_interest.py compares the kernels
with: the float64 arg-max over k (lowest k on a tie) of  table · gelu(mui · W2ᵀ)ᵀ  ('weighted': the
logits under the target-aware softmax, model.py:212-213), respectively  table · muiᵀ  ('max',
model.py:127-129) — and the decisive-pair rule that goes with it:

    b = rtol · |top| + floor · rms     (rms over all the logits, respectively all M, of the world;
                                        the project's bars: fp32 1e-5 / 1e-5, 16-bit 2e-4 / 2e-4)
    a pair is decisive iff the gap between its two largest values exceeds 2 b.

Both values of a pair carry an error of at most b in the format the bar belongs to, so a decisive
pair's arg-max cannot differ from the float64 one: it must match exactly, and an undecided pair is
skipped. What may be skipped is bounded here, without a GPU: at most 2 % of a golden user's pairs
(users with at least 37 clicks; the all-padded and the 1-3-click users have near-identical interests
and are checked on their decisive pairs only), at most 1 % of a user's pairs in the random worlds of
tests/test_gpu_corpus_rankof.py (same seeds, rebuilt on the CPU).
"""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
F32_TOL = dict(rtol=1e-5, rms_floor=1e-5)          # the bars of tests/test_gpu_corpus_rankof.py
RANK16_TOL = dict(rtol=2e-4, rms_floor=2e-4)
MIN_CLICKS = 37                                     # golden users with at least this many clicks: the share bound holds
GOLDEN = ("c5_weighted", "c5_max")


def gelu64(x):
    return torch.nn.functional.gelu(torch.as_tensor(x, dtype=torch.float64)).numpy()


def interest_values(table, rows):
    """[U, N, K] float64: table · rowsᵀ per user — rows = proj [U, K, d] ('weighted') or mui ('max')."""
    return np.einsum("nd,ukd->unk", np.asarray(table, np.float64), np.asarray(rows, np.float64))


def dominant(V, tol):
    """V [U, N, K] float64 -> (arg [U, N] the lowest k at the maximum, gap [U, N] between the two
    largest values, decisive [U, N] bool, b [U, N]) under the decisive-pair rule at the bar ``tol``."""
    arg = V.argmax(axis=2)                                       # numpy: the first (lowest) index of the maximum
    two = np.sort(V, axis=2)[:, :, -2:]
    gap = two[:, :, 1] - two[:, :, 0]
    rms = float(np.sqrt(np.mean(V ** 2)))
    b = tol["rtol"] * np.abs(two[:, :, 1]) + tol["rms_floor"] * rms
    return arg, gap, gap > 2 * b, b


def load(name):
    z = np.load(os.path.join(HERE, "golden", f"corpus_{name}.npz"), allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["score_type"] = str(g["score_type"])
    zi = np.load(os.path.join(HERE, "golden", "interest", f"corpus_interest_{name}.npz"), allow_pickle=False)
    g.update(interest=zi["interest"], margin=zi["margin"], interest_scores=zi["scores"])
    g["clicks"] = g["his_mask"].sum(axis=1)
    return g


def golden_values(g):
    """The float64 restatement on a fixture: from the reference's mui (and W2)."""
    if g["score_type"] == "weighted":
        proj = gelu64(np.einsum("ukd,ed->uke", g["mui"].astype(np.float64), g["W2"].astype(np.float64)))
        return interest_values(g["table"], proj)
    return interest_values(g["table"], g["mui"])


def check_against_golden(got, g, tol, what):
    """``got`` [U, N] interests against the fixture's under the decisive-pair rule at ``tol``; returns
    the share of undecided pairs per user."""
    _, _, decisive, _ = dominant(golden_values(g), tol)
    got = np.asarray(got)
    assert got.shape == g["interest"].shape, what
    bad = decisive & (got != g["interest"])
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist())
    return 1.0 - decisive.mean(axis=1)


@pytest.mark.parametrize("name", GOLDEN)
def test_the_fixture_is_the_case(name):
    g = load(name)
    assert np.array_equal(g["interest_scores"], g["scores"])     # the same model, table and histories
    U, N, K = int(g["U"]), int(g["N"]), int(g["K"])
    assert g["interest"].shape == g["margin"].shape == (U, N) and g["interest"].dtype == np.int32
    assert (g["interest"] >= 0).all() and (g["interest"] < K).all() and (g["margin"] >= 0).all()


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_matches_the_reference(name):
    """The float64 arg-max equals the reference's own on every decisive pair (fp32 bar: the reference
    computes in fp32), and its top-two gap is the reference's margin: both values of the pair carry
    at most b, so the gap at most 2 b — plus, for 'weighted', the fp32 softmax, divide and log that
    turn the two weights into the recorded log-ratio, a few 2^-24 relative each: 1e-6 (absolute on the
    log) covers them."""
    g = load(name)
    V = golden_values(g)
    arg, gap, decisive, b = dominant(V, F32_TOL)
    assert (arg[decisive] == g["interest"][decisive]).all()
    assert decisive.mean() > 0.5
    err = np.abs(gap - g["margin"].astype(np.float64))
    bound = 2 * b + 1e-6 + 2.0 ** -23 * np.abs(gap)             # (the margin itself is stored in fp32)
    print(name, "max |gap - margin| / bound", float((err / bound).max()), "undecided per user", (1 - decisive.mean(axis=1)).round(4))
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("name", GOLDEN)
def test_what_the_golden_tests_may_skip(name):
    """At most 2 % of a user's pairs at the fp32 bar (the golden tests run in fp32), for the users
    with at least 37 clicks. Measured: 0.43 / 1.29 / 0.57 % (c5_weighted), 0.33 / 0.83 % (c5_max); the
    all-padded and the 1-3-click users: 7.7 - 100 %, no bound."""
    g = load(name)
    undecided = 1.0 - dominant(golden_values(g), F32_TOL)[2].mean(axis=1)
    print(name, "undecided per user", undecided.round(4), "clicks", g["clicks"])
    assert (undecided[g["clicks"] >= MIN_CLICKS] <= 0.02).all(), undecided
    assert (g["clicks"] >= MIN_CLICKS).sum() >= 2


def cpu_world(shape):
    """tests/test_gpu_corpus_rankof.py's random users and table of ``shape`` rebuilt on the CPU (the
    same generator calls, rounded to the shape's dtype): (mui, proj, table) float32 — what the GPU
    tests' world holds on the device."""
    import test_gpu_corpus_rankof as base
    U, K, d, N, dtype = base.SHAPES[shape]
    gen = torch.Generator().manual_seed(7 + len(shape) + K + N)
    mui = torch.randn(U, K, d, generator=gen) / 2
    proj = torch.randn(U, K, d, generator=gen) / 2
    table = torch.randn(N, d, generator=gen) / d ** 0.5
    table[N // 2:N // 2 + base.DUP] = table[:base.DUP]
    return tuple(x.to(dtype).float().numpy() for x in (mui, proj, table))


def test_what_the_world_tests_may_skip():
    """At most 1 % of a user's N pairs in every base.CASES world with a dominant interest, at the
    16-bit bar (the wider one)."""
    import test_gpu_corpus_rankof as base
    for shape, score_type in base.CASES + [("mid_f16", "max"), ("k20_f16", "max")]:
        if score_type == "mean":
            continue
        mui, proj, table = cpu_world(shape)
        V = interest_values(table, proj if score_type == "weighted" else mui)
        undecided = 1.0 - dominant(V, RANK16_TOL)[2].mean(axis=1)
        print(shape, score_type, "undecided per user", undecided.round(4))
        assert (undecided <= 0.01).all(), (shape, score_type, undecided)
