"""The options of the ranking entries, checked in one place: one table of bad option sets — every
combination rule (after with caps; resume with after, or without a cap; the two kinds of caps
together; 'mean' with interests; user_group without news_bias; one of news_cluster / cluster_cap
without the other) and a wrong dtype, rank or length of every tensor option — goes through every
entry that takes the options: rank_topk, rank_topk_deep, rank_topk_deep_capped, rank_corpus and
update_topk. On CPU tensors each bad set raises ValueError, the same class through every entry, and
its well-formed counterpart RuntimeError (there is no CPU path): the argument errors come before the
device check. The filters that are converted on the device (exclude_ids, eligible, news_ids) have
their bad values in tests/test_gpu_corpus_request.py, on device tensors. No compute call is made
(runs on CPU-only machines)."""
import dataclasses
import inspect

import pytest
import torch

from miner_amd import corpus

U, K, D, N, L = 3, 4, 64, 50, 6
MUI = torch.zeros(U, K, D)
TAB = torch.zeros(N, D)
HID, MASK = torch.zeros(U, L, dtype=torch.int32), torch.ones(U, L, dtype=torch.bool)
PK = corpus.EncoderWeights(torch.zeros(16, dtype=torch.uint8), torch.float32, D, 8, K, True)
IDS = torch.zeros(U, 5, dtype=torch.int64)
PAIR, TRIPLE = (torch.zeros(U, 5), IDS), (torch.zeros(U, 5), IDS, IDS.int())
CLUS = torch.arange(N) % 4
CAPS = dict(news_cluster=CLUS, cluster_cap=2)
CAP_KEYS = ("news_cluster", "cluster_cap", "interest_cap")
PRIOR1, PRIOR2 = torch.zeros(N), torch.zeros(2, N)
GRP = torch.arange(U) % 2
CUR = corpus.start_cursor(U, "cpu")
STATE = corpus.start_walk(U, "cpu", 4)
rep = dataclasses.replace

ENTRIES = {
    "rank_topk": lambda lists, **kw: corpus.rank_topk(MUI, MUI, TAB, 5, **kw),
    "rank_topk_deep": lambda lists, **kw: corpus.rank_topk_deep(MUI, MUI, TAB, 300, **kw),
    "rank_topk_deep_capped": lambda lists, **kw: corpus.rank_topk_deep_capped(MUI, MUI, TAB, 300, **kw),
    "rank_corpus": lambda lists, **kw: corpus.rank_corpus(TAB, HID, MASK, PK, 5, **kw),
    "update_topk": lambda lists, **kw: corpus.update_topk(lists, MUI, MUI, TAB, IDS[0], **kw),
}


def case(good, *bad):
    return [(b, good) for b in bad]


# (bad options, their well-formed counterpart)
TABLE = [
    # the combination rules
    *case(dict(after=CUR), dict(after=CUR, **CAPS), dict(after=CUR, news_cluster=CLUS), dict(after=CUR, cluster_cap=2)),
    *case(dict(interest_cap=2, score_type="max"), dict(interest_cap=2, after=CUR)),
    *case(dict(resume=STATE, **CAPS), dict(resume=STATE, after=CUR, **CAPS), dict(resume=STATE)),
    *case(dict(resume=STATE, interest_cap=2), dict(resume=STATE, interest_cap=2, after=CUR),
          dict(resume=STATE, return_interest=True), dict(resume=STATE, interest_cap=2, **CAPS)),
    *case(dict(interest_cap=2), dict(interest_cap=2, **CAPS), dict(interest_cap=2, news_cluster=CLUS),
          dict(interest_cap=2, cluster_cap=2), dict(interest_cap=2, score_type="mean")),
    *case(dict(return_interest=True), dict(return_interest=True, score_type="mean")),
    *case(dict(user_group=GRP, news_bias=PRIOR2), dict(user_group=GRP)),
    *case(dict(**CAPS), dict(news_cluster=CLUS), dict(cluster_cap=2)),
    # the caps' values
    *case(dict(**CAPS), *(dict(news_cluster=CLUS, cluster_cap=c) for c in (0, -1, corpus.MAX_TOPK + 1, 2.0, "2", True))),
    *case(dict(interest_cap=corpus.MAX_TOPK), *(dict(interest_cap=c) for c in (0, -1, corpus.MAX_TOPK + 1, 2.0, "2", True))),
    # a wrong dtype, rank or length of each tensor option
    *case(dict(news_bias=PRIOR1), dict(news_bias=PRIOR1.double()), dict(news_bias=PRIOR1.long()),
          dict(news_bias=torch.zeros(1, 1, N)), dict(news_bias=torch.zeros(N + 1)), dict(news_bias=torch.zeros(0, N)),
          dict(news_bias=PRIOR2), dict(news_bias=PRIOR1.tolist())),
    *case(dict(news_bias=PRIOR2, user_group=GRP), dict(news_bias=PRIOR2, user_group=GRP.float()),
          dict(news_bias=PRIOR2, user_group=GRP == 0), dict(news_bias=PRIOR2, user_group=GRP[None, :]),
          dict(news_bias=PRIOR2, user_group=torch.zeros(U + 1, dtype=torch.int64)),
          dict(news_bias=PRIOR2, user_group=GRP + 1), dict(news_bias=PRIOR2, user_group=GRP - 1)),
    *case(dict(**CAPS), dict(news_cluster=CLUS.float(), cluster_cap=2), dict(news_cluster=CLUS == 0, cluster_cap=2),
          dict(news_cluster=CLUS[None, :], cluster_cap=2), dict(news_cluster=torch.zeros(N + 1, dtype=torch.int32), cluster_cap=2),
          dict(news_cluster=CLUS + 2 ** 40, cluster_cap=2)),
    *case(dict(after=CUR), dict(after=(CUR[0].double(), CUR[1])), dict(after=(CUR[0], CUR[1].float())),
          dict(after=(CUR[0][None, :], CUR[1])), dict(after=(CUR[0], CUR[1][None, :])), dict(after=(CUR[0][:2], CUR[1][:2])),
          dict(after=(CUR[0], CUR[1].long() + 2 ** 40)), dict(after=CUR[0]), dict(after=(CUR[0],)), dict(after=3)),
    *case(dict(resume=STATE, **CAPS), *(dict(resume=bad, **CAPS) for bad in (
        CUR, 3, rep(STATE, scores=STATE.scores.double()), rep(STATE, scores=STATE.scores[None, :]),
        rep(STATE, scores=STATE.scores[:2]), rep(STATE, ids=STATE.ids.long()), rep(STATE, ids=STATE.ids[:2]),
        rep(STATE, groups=STATE.groups.long()), rep(STATE, groups=STATE.groups[0], counts=STATE.counts[0]),
        rep(STATE, counts=STATE.counts[:, :3]), rep(STATE, n_used=STATE.n_used.long()), rep(STATE, n_used=STATE.n_used[:2]),
        rep(STATE, overflow=STATE.overflow.bool()), rep(STATE, overflow=STATE.overflow[:2]), corpus.start_walk(U + 1, "cpu", 4)))),
]


def params(name):
    return set(inspect.signature(getattr(corpus, name)).parameters)


def applies(name, bad, good):
    """Whether the entry offers the options of the bad set and of its well-formed counterpart."""
    if not set(bad) | set(good) <= params(name):
        return False
    if name == "rank_topk_deep":              # pages with cursors: the cap options are named only to refuse them
        return not any(k in good for k in CAP_KEYS)
    if name == "rank_topk_deep_capped":       # the interests are listed under interest_cap only
        return "interest_cap" in good or not good.get("return_interest")
    return True


def run(name, kw, good):
    if name == "rank_topk_deep_capped" and not any(k in good for k in CAP_KEYS):
        kw = dict(kw, **CAPS)                 # the capped walk: a case about something else runs under caps
    # update_topk's lists carry interests exactly when the options ask for them
    return ENTRIES[name](TRIPLE if "interest_cap" in kw else PAIR, **kw)


def asked(name):
    return [(bad, good) for bad, good in TABLE if applies(name, bad, good)]


@pytest.mark.parametrize("name", list(ENTRIES))
def test_bad_options_raise_valueerror_before_the_device_check(name):
    for bad, good in asked(name):
        with pytest.raises(ValueError) as e:
            run(name, bad, good)
        assert type(e.value) is ValueError, (name, bad)      # the same class through every entry
        with pytest.raises(RuntimeError, match="GPU only"):
            run(name, good, good)


def test_every_rule_reaches_every_entry_that_takes_its_options():
    """``applies`` does not narrow the table silently: each rule is asked of the entries named here."""
    keys = {name: {frozenset(bad) for bad, _ in asked(name)} for name in ENTRIES}
    caps = {"news_cluster", "cluster_cap"}
    want = [
        ({"after"} | caps, ("rank_topk", "rank_corpus", "rank_topk_deep")),
        ({"after"}, ("rank_topk", "rank_corpus", "rank_topk_deep")),
        ({"resume", "after"} | caps, ("rank_topk", "rank_corpus")),
        ({"resume"}, ("rank_topk", "rank_corpus", "rank_topk_deep_capped")),
        ({"resume"} | caps, ("rank_topk", "rank_corpus", "rank_topk_deep_capped")),
        ({"interest_cap"} | caps, ("rank_topk", "rank_corpus", "rank_topk_deep_capped", "update_topk")),
        ({"interest_cap", "score_type"}, ("rank_topk", "rank_corpus", "rank_topk_deep_capped", "update_topk")),
        ({"return_interest", "score_type"}, ("rank_topk", "rank_corpus", "rank_topk_deep")),
        ({"news_cluster"}, ("rank_topk", "rank_corpus", "rank_topk_deep_capped", "update_topk")),
        ({"cluster_cap"}, ("rank_topk", "rank_corpus", "rank_topk_deep_capped", "update_topk")),
        (caps, ("rank_topk", "rank_corpus", "rank_topk_deep_capped", "update_topk")),
        ({"user_group"}, tuple(ENTRIES)),
        ({"news_bias"}, tuple(ENTRIES)),
        ({"news_bias", "user_group"}, tuple(ENTRIES)),
    ]
    for options, names in want:
        for name in names:
            assert frozenset(options) in keys[name], (sorted(options), name)
    assert {name: len(asked(name)) for name in ENTRIES} == {"rank_topk": 71, "rank_corpus": 71, "rank_topk_deep": 27,
                                                            "rank_topk_deep_capped": 55, "update_topk": 37}
