"""corpus_metrics (miner_amd/corpus.py) against the reference's per-impression metric functions as
miner_amd/evaluation.py mirrors them: 20 users over N = 50 surviving news with distinct float64
scores (the reference functions break ties in other ways than the ranker) and 1-4 targets each;
the ranks come from numpy's lexsort, the yardsticks from the dense y_true / y_score. Pure torch on
the CPU."""
import numpy as np
import pytest
import torch

from miner_amd import corpus
from miner_amd.evaluation import auc_score, compute_mrr_score, compute_ndcg_score, is_hit

U, N, T, KS = 20, 50, 4, (1, 5, 10)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(11)
    scores = rng.permuted(np.tile(np.linspace(-1.0, 1.0, N), (U, 1)), axis=1) + rng.uniform(-1e-3, 1e-3, (U, N))
    assert all(len(np.unique(scores[u])) == N for u in range(U))
    ranks = np.full((U, T), -1, np.int64)
    y_true = np.zeros((U, N))
    for u in range(U):
        m = 1 + u % T
        tgt = rng.choice(N, size=m, replace=False)
        order = np.lexsort((np.arange(N), -scores[u]))            # the ranker's order: score desc, id asc
        pos = np.empty(N, np.int64)
        pos[order] = np.arange(N)
        slots = rng.choice(T, size=m, replace=False)              # the targets in any slots, -1 elsewhere
        ranks[u, slots] = pos[tgt]
        y_true[u, tgt] = 1.0
    if not (ranks[0] == 0).any():                                 # one user with a target at rank 0 ...
        u = 0
        y_true[u] = 0.0
        y_true[u, np.argmax(scores[u])] = 1.0
        ranks[u] = [-1, 0, -1, -1]
    u = 1                                                         # ... and one with its target last
    y_true[u] = 0.0
    y_true[u, np.argmin(scores[u])] = 1.0
    ranks[u] = [N - 1, -1, -1, -1]
    return scores, y_true, ranks


def test_against_the_reference_functions(case):
    scores, y_true, ranks = case
    per, means = corpus.corpus_metrics(torch.from_numpy(ranks), torch.full((U,), N), ks=KS)
    want = {"mrr": [compute_mrr_score(y_true[u], scores[u]) for u in range(U)],
            "auc": [auc_score(y_true[u], scores[u]) for u in range(U)]}
    for k in KS:
        want[f"ndcg@{k}"] = [compute_ndcg_score(y_true[u], scores[u], k) for u in range(U)]
        want[f"hit@{k}"] = [float(is_hit(y_true[u], scores[u], k)) for u in range(U)]
        want[f"recall@{k}"] = [sum(1 for r in ranks[u] if 0 <= r < k) / sum(1 for r in ranks[u] if r >= 0)
                               for u in range(U)]
    assert set(per) == set(want) == set(means)
    for name, w in want.items():
        got = per[name].numpy()
        assert got.dtype == np.float64
        assert np.abs(got - np.asarray(w)).max() <= 1e-12, name
        assert abs(means[name] - float(np.mean(w))) <= 1e-12, name


def test_int32_ranks_and_no_survivor_count(case):
    _, _, ranks = case
    a, ma = corpus.corpus_metrics(torch.from_numpy(ranks), ks=KS)
    b, mb = corpus.corpus_metrics(torch.from_numpy(ranks).to(torch.int32), torch.full((U,), N, dtype=torch.int32), ks=KS)
    assert "auc" not in a and "auc" in b
    for name in a:
        assert torch.equal(a[name], b[name]) and ma[name] == mb[name]


def test_users_without_a_target_are_left_out(case):
    _, _, ranks = case
    r = torch.from_numpy(ranks)
    n = torch.full((U,), N)
    extra = torch.cat([r, torch.full((3, T), -1)], dim=0)         # three users with no target at all
    per, means = corpus.corpus_metrics(extra, torch.cat([n, n[:3]]), ks=KS)
    _, base = corpus.corpus_metrics(r, n, ks=KS)
    for name in base:
        assert torch.isnan(per[name][U:]).all(), name
        assert abs(means[name] - base[name]) <= 1e-12, name
    _, none = corpus.corpus_metrics(torch.full((2, T), -1), ks=KS)
    assert all(np.isnan(v) for v in none.values())


def test_auc_is_undefined_where_every_ranked_news_is_a_target():
    per, means = corpus.corpus_metrics(torch.tensor([[0, 1], [1, 0], [2, -1]]), torch.tensor([2, 5, 3]), ks=(1,))
    assert torch.isnan(per["auc"][0])
    assert per["auc"][1].item() == 1.0 and per["auc"][2].item() == 0.0
    assert means["auc"] == 0.5
