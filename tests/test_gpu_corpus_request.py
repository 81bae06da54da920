"""The ranking entries behind one request — needs an MI355X. Nothing here has a yardstick of its
own: every check is one entry against another entry (or its own pages chained by hand), bit for bit,
under all the options at once, so that what an entry hands on, slices per batch or replaces per
page is what rank_topk itself gets. The scores' own correctness is the other corpus tests' matter.

Shapes: U = 5 (a tile with a user past U; with batch=2 a one-user batch), K = 40 in fp16 with
d = 128 (two interest tiles) and K = 8 in fp32 with d = 64, N = 300 (one full and one partial news
step); MINER_RK_SPLIT = 0 and 1 where the form has a split (the capped forms have none)."""
import functools

import pytest
import torch

from miner_amd import corpus, synthetic

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:rank_topk. topk=:RuntimeWarning")]
DEV = "cuda:0"
U, N, L, TOPK = 5, 300, 12, 7
CASES = {"f16_k40": (torch.float16, 40, 128), "f32_k8": (torch.float32, 8, 64)}
SPLITS = ("0", "1")


@functools.lru_cache(maxsize=None)
def world(case):
    dtype, K, d = CASES[case]
    g = torch.Generator().manual_seed(K)
    z = dict(K=K)
    z["t"] = (torch.randn(N, d, generator=g) / d ** 0.5).to(DEV, dtype)
    z["hid"] = torch.randint(0, N, (U, L), generator=g).to(DEV)
    z["mask"] = (torch.rand(U, L, generator=g) > 0.2).to(DEV)
    z["mask"][:, 0] = True
    W1, Q, W2 = synthetic.init_weights(K, d, 48, K, device=DEV)
    z["pk"] = corpus.pack_encoder(W1, Q, W2, dtype=dtype)
    z["m"], z["p"] = corpus.encode_users(z["t"], z["mask"], z["pk"], his_ids=z["hid"])
    excl = torch.randint(0, N, (U, 6), generator=g)
    excl[:, 4:] = -1                                                     # padding
    excl[0, 0], excl[1, 1] = N + 5, -7                                   # ... and ids that exclude nothing
    raw = torch.randint(-20, N + 20, (2000,), generator=g)              # unsorted, repeats, out of range
    clus = torch.arange(N) % 11
    clus[torch.randperm(N, generator=g)[:20]] = -1                       # in no cluster
    fine = torch.arange(N)                                               # lists deeper than a page: 8 clusters of 3
    fine[:24] = torch.arange(24) % 8
    # every option that combines with every other
    z["opts"] = dict(exclude_ids=excl.to(DEV), eligible=(torch.rand(N, generator=g) < 0.97).to(DEV),
                     news_bias=(0.5 * torch.randn(2, N, generator=g)).to(DEV), user_group=(torch.arange(U) % 2).to(DEV))
    z["raw"] = raw.to(DEV)
    z["caps"] = dict(news_cluster=clus.to(DEV), cluster_cap=1)
    z["fine"] = fine.to(DEV)
    return z


def same(got, want, what=""):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what           # bit for bit


def same_state(a, b):
    same((a.scores, a.ids, a.groups, a.counts, a.n_used, a.overflow.int()),
         (b.scores, b.ids, b.groups, b.counts, b.n_used, b.overflow.int()))


def two_pages_in(z, capkw, **kw):
    """The state after two pages of a capped walk under the options, and the pages' widths."""
    state = corpus.start_walk(U, DEV, 512)
    for k in (3, 2):
        page = corpus.rank_topk(z["m"], z["p"], z["t"], k, resume=state, **capkw, **kw)
        state = corpus.advance_walk(state, page, news_cluster=capkw.get("news_cluster"))
    assert bool((state.n_used > 0).all()) and not bool(state.overflow.any())
    return state


def rest(z, kind):
    """The options besides the filters and the prior: caps with a state two pages into the walk, the
    interest cap with one, or (the forms that split) a cursor."""
    kw = dict(z["opts"], news_ids=z["raw"])
    if kind == "caps":
        return dict(kw, **z["caps"], resume=two_pages_in(z, z["caps"], **kw))
    if kind == "interests":
        capkw = dict(interest_cap=2, return_interest=True)
        return dict(kw, **capkw, resume=two_pages_in(z, capkw, **kw))
    first = corpus.rank_topk(z["m"], z["p"], z["t"], 4, **kw)
    return dict(kw, after=corpus.page_cursor(first), return_interest=kind == "cursor_interests")


@pytest.mark.parametrize("kind,split", [("caps", ""), ("interests", "")] + [(k, s) for k in ("cursor", "cursor_interests")
                                                                              for s in SPLITS])
@pytest.mark.parametrize("case", list(CASES))
def test_rank_corpus_in_batches_is_rank_topk_on_all_users(case, kind, split, monkeypatch):
    monkeypatch.setenv("MINER_RK_SPLIT", split)
    z = world(case)
    kw = rest(z, kind)
    want = corpus.rank_topk(z["m"], z["p"], z["t"], TOPK, **kw)
    assert bool((want[1][:, 0] >= 0).all()) and len(want) == (2 if kind in ("caps", "cursor") else 3)
    plain = corpus.rank_topk(z["m"], z["p"], z["t"], TOPK)
    assert not torch.equal(want[1], plain[1])                            # the options bite
    same(corpus.rank_corpus(z["t"], z["hid"], z["mask"], z["pk"], TOPK, batch=2, **kw), want, "batch=2")
    same(corpus.rank_corpus(z["t"], z["hid"], z["mask"], z["pk"], TOPK, batch=U, **kw), want, "one batch")
    # the per-user slicing by hand: users 1 .. 3 with every per-user option sliced
    cut = dict(kw, exclude_ids=kw["exclude_ids"][1:4], user_group=kw["user_group"][1:4])
    if "resume" in kw:
        cut["resume"] = kw["resume"].users(1, 4)
    else:
        cut["after"] = tuple(t[1:4] for t in kw["after"])
    same(corpus.rank_topk(z["m"][1:4], z["p"][1:4], z["t"], TOPK, **cut), tuple(t[1:4] for t in want), "users 1..3")
    # exclude_history: the history joins the exclusion matrix
    seen = torch.where(z["mask"], z["hid"], -1)
    same(corpus.rank_corpus(z["t"], z["hid"], z["mask"], z["pk"], TOPK, batch=2, exclude_history=True, **kw),
         corpus.rank_topk(z["m"], z["p"], z["t"], TOPK, **dict(kw, exclude_ids=torch.cat([seen, kw["exclude_ids"]], dim=1))))


@pytest.mark.parametrize("capkw", [dict(cluster_cap=2), dict(interest_cap=40, return_interest=True)], ids=["caps", "interests"])
@pytest.mark.parametrize("case", list(CASES))
def test_deep_capped_is_its_pages_chained_with_advance_walk(case, capkw):
    z = world(case)
    kw = dict(z["opts"], news_ids=z["raw"])
    if "cluster_cap" in capkw:
        capkw = dict(capkw, news_cluster=z["fine"])
    clus = capkw.get("news_cluster")
    state = s0 = two_pages_in(z, capkw, **kw)
    pages = []
    for k in (256, 4):
        pages.append(corpus.rank_topk(z["m"], z["p"], z["t"], k, resume=state, **capkw, **kw))
        state = corpus.advance_walk(state, pages[-1], news_cluster=clus)
    want = tuple(torch.cat(ts, dim=1) for ts in zip(*pages))
    assert clus is None or bool((want[1][:, 256] >= 0).any())            # the second page lists something
    got = corpus.rank_topk_deep_capped(z["m"], z["p"], z["t"], 260, resume=s0, return_state=True, **capkw, **kw)
    same(got[:-1], want)
    same_state(got[-1], state)
    same(corpus.rank_topk_deep_capped(z["m"], z["p"], z["t"], 260, resume=s0, **capkw, **kw), want)
    # from the top: start_walk of the given capacity
    first = corpus.rank_topk(z["m"], z["p"], z["t"], 256, **capkw, **kw)
    top = corpus.rank_topk_deep_capped(z["m"], z["p"], z["t"], 260, capacity=300, **capkw, **kw)
    same(tuple(t[:, :256] for t in top), first)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("interests", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_deep_is_its_pages_chained_with_page_cursor(case, interests, split, monkeypatch):
    monkeypatch.setenv("MINER_RK_SPLIT", split)
    z = world(case)
    kw = dict(z["opts"], news_ids=z["raw"], return_interest=interests)
    cur = corpus.page_cursor(corpus.rank_topk(z["m"], z["p"], z["t"], 3, **kw)[:2])
    p1 = corpus.rank_topk(z["m"], z["p"], z["t"], 256, after=cur, **kw)
    p2 = corpus.rank_topk(z["m"], z["p"], z["t"], 4, after=corpus.page_cursor(p1[:2]), **kw)
    want = tuple(torch.cat(ts, dim=1) for ts in zip(p1, p2))
    assert bool((want[1][:, 256] >= 0).any())                            # the second page lists something
    same(corpus.rank_topk_deep(z["m"], z["p"], z["t"], 260, after=cur, **kw), want)


@pytest.mark.parametrize("kind", ["plain", "caps", "interests"])
@pytest.mark.parametrize("case", list(CASES))
def test_update_topk_is_merge_topk_of_rank_topk(case, kind):
    z = world(case)
    capkw = dict(plain={}, caps=z["caps"], interests=dict(interest_cap=2))[kind]
    ret = dict(return_interest=True) if kind == "interests" else {}
    old_ids, new_ids = z["raw"][:200], z["raw"][200:]
    old = corpus.rank_topk(z["m"], z["p"], z["t"], TOPK, news_ids=old_ids, **z["opts"], **capkw, **ret)
    fresh = corpus.rank_topk(z["m"], z["p"], z["t"], TOPK, news_ids=new_ids, **z["opts"], **capkw, **ret)
    want = corpus.merge_topk(old, fresh, TOPK, eligible=z["opts"]["eligible"], **capkw)
    assert not torch.equal(want[1], old[1])                              # the fresh rows enter the lists
    same(corpus.update_topk(old, z["m"], z["p"], z["t"], new_ids, **z["opts"], **capkw), want)


def test_the_list_is_canonicalised_and_the_bitmap_packed_once_per_call(monkeypatch):
    z = world("f32_k8")
    calls = dict(ids=0, bits=0)
    canon, pack = corpus.canonical_news_ids, corpus.pack_eligible

    def count_ids(*a, **kw):
        calls["ids"] += 1
        return canon(*a, **kw)

    def count_bits(*a, **kw):
        calls["bits"] += 1
        return pack(*a, **kw)

    monkeypatch.setattr(corpus, "canonical_news_ids", count_ids)
    monkeypatch.setattr(corpus, "pack_eligible", count_bits)
    kw = dict(z["opts"], news_ids=z["raw"])
    runs = {
        "rank_corpus, 3 batches": lambda: corpus.rank_corpus(z["t"], z["hid"], z["mask"], z["pk"], TOPK, batch=2, **kw),
        "rank_corpus, 5 batches, caps": lambda: corpus.rank_corpus(z["t"], z["hid"], z["mask"], z["pk"], TOPK, batch=1, **kw,
                                                                   **z["caps"]),
        "rank_topk_deep, 2 pages": lambda: corpus.rank_topk_deep(z["m"], z["p"], z["t"], 260, **kw),
        "rank_topk_deep_capped, 2 pages": lambda: corpus.rank_topk_deep_capped(z["m"], z["p"], z["t"], 260, **kw,
                                                                               news_cluster=z["fine"], cluster_cap=2),
        "rank_topk": lambda: corpus.rank_topk(z["m"], z["p"], z["t"], TOPK, **kw),
    }
    for what, run in runs.items():
        calls.update(ids=0, bits=0)
        run()
        assert calls == dict(ids=1, bits=1), what


def test_bad_filters_raise_valueerror_through_every_entry():
    """The filters' own argument errors (tests/test_corpus_request_host.py has the other options'),
    on device tensors: the same class through every entry."""
    z = world("f32_k8")
    excl, ok = z["opts"]["exclude_ids"], z["opts"]["eligible"]
    entries = {
        "rank_topk": lambda news_ids=None, **kw: corpus.rank_topk(z["m"], z["p"], z["t"], TOPK, news_ids=news_ids, **kw),
        "rank_topk_deep": lambda news_ids=None, **kw: corpus.rank_topk_deep(z["m"], z["p"], z["t"], 260, news_ids=news_ids, **kw),
        "rank_topk_deep_capped": lambda news_ids=None, **kw: corpus.rank_topk_deep_capped(
            z["m"], z["p"], z["t"], 260, news_ids=news_ids, **z["caps"], **kw),
        "rank_corpus": lambda news_ids=None, **kw: corpus.rank_corpus(z["t"], z["hid"], z["mask"], z["pk"], TOPK, batch=2,
                                                                      news_ids=news_ids, **kw),
        "update_topk": lambda news_ids=z["raw"], **kw: corpus.update_topk(
            corpus.rank_topk(z["m"], z["p"], z["t"], TOPK), z["m"], z["p"], z["t"], news_ids, **kw),
    }
    bad = [dict(exclude_ids=excl.float()), dict(exclude_ids=excl[0]), dict(exclude_ids=excl[:3]),
           dict(exclude_ids=torch.zeros(U, corpus.MAX_L + 1, dtype=torch.int32, device=DEV)),
           dict(eligible=ok[:-1]), dict(eligible=ok.long()), dict(eligible=ok[None, :]),
           dict(eligible=corpus.pack_eligible(ok)[:-1]),
           dict(news_ids=z["raw"].float()), dict(news_ids=z["raw"][None, :]), dict(news_ids=z["raw"] >= 0),
           dict(news_ids=corpus.canonical_news_ids(z["raw"], N + 1))]
    for name, call in entries.items():
        for kw in bad:
            with pytest.raises(ValueError) as e:
                call(**kw)
            assert type(e.value) is ValueError, (name, list(kw))
        call(exclude_ids=excl, eligible=corpus.pack_eligible(ok), news_ids=corpus.canonical_news_ids(z["raw"], N))
