"""Full-corpus ranking on MI355X (BASELINE config 5: 1M users x 200k news, history 200, K=64,
d=768, fp16), backed by libminer_hip.so (include/miner_corpus.h).

    packed = pack_encoder(w_poly, context_codes, w_target, dtype=torch.float16)
    mui, proj = encode_users(history, his_mask, packed)                 # or table + his_ids
    top_scores, top_ids = rank_topk(mui, proj, news_table, topk=100)   # never materialises U x N
    rank_topk(..., exclude_ids=clicked, eligible=fresh)    # per-user "not these", table-wide "only these"
    rank_topk(..., news_ids=new_rows)                      # only these rows are read: cost by their count
    lists = update_topk(lists, mui, proj, news_table, new_rows)   # ... and folded into served lists
    scores = score_pairs(mui, proj, news_table, cand_ids)  # [U, C] chosen pairs, the ranker's own bits
    ranks, scores = rank_of(mui, proj, news_table, clicked, exclude_ids=history)   # exact ranks among all N
    per_user, means = corpus_metrics(ranks, n_ranked)      # recall@k / hit@k / ndcg@k / mrr / auc
    ranks, metrics = evaluate_corpus(news_table, his_ids, his_mask, packed, clicked)  # the full-ranking protocol
    lists = rescore_topk(lists, new_mui, new_proj, news_table)    # served lists after the users changed
    rank_topk(..., news_bias=prior)                        # fp32 [N] or [G, N] (+ user_group [U]) added to the
                                                           # click score before it ranks; also score_pairs, rank_of,
                                                           # update_topk, rescore_topk, rank_corpus, evaluate_corpus
    page2 = rank_topk(..., after=page_cursor(page1))       # keyset cursors: the ranking continued strictly after
                                                           # (score, id) per user; start_cursor, page_cursor;
    deep = rank_topk_deep(mui, proj, news_table, 1000)     # any depth, ceil(topk / 256) pages side by side
    rank_topk(..., news_cluster=story, cluster_cap=1)      # at most cluster_cap news of one cluster (int [N], < 0:
                                                           # none) per list, inside the ranker's merge; also merge_topk,
                                                           # update_topk, rank_corpus; cap_topk(lists, story, 1) caps a
                                                           # served list (unsplit kernel only; not rank_of / score_pairs)
    s, i, g = rank_topk(..., return_interest=True)         # g int32 [U,topk]: which of the user's K interests each
                                                           # listed news matched (the arg-max of the score's own
                                                           # reduction over K; 'weighted' / 'max'); also score_pairs,
    rank_topk(..., interest_cap=3, return_interest=True)   # rank_topk_deep, rank_corpus. At most interest_cap news of one
                                                           # dominant interest per list; triples through merge_topk /
                                                           # update_topk(interest_cap=) (unsplit kernel only, no cursor;
                                                           # not rank_of / evaluate_corpus / rescore_topk)
    state = start_walk(U, device)                          # the cursor under caps: a WalkState carries the cursor and
    page = rank_topk(..., cluster_cap=1, resume=state)     # the per-group counts of the pages served so far;
    state = advance_walk(state, page, news_cluster=story)  # advanced on the device; also rank_corpus(resume=) and
    deep = rank_topk_deep_capped(..., 1000, cluster_cap=1) # capped lists of any depth (not merge_topk / update_topk / cap_topk)
    page = diversify_topk(pool, news_table, 50, lam=0.7)   # diversity re-ranking (MMR) of a ranked pool of <= 256 entries
    page = rank_topk_diverse(mui, proj, news_table, 50)    # by the table's own cosine similarity; rank_topk + diversify_topk

The click score of (user, news) is the reference's (src/model/model.py:127-134, 213-214) with the
impression's candidate set replaced by the whole news table; ties rank the lower news id first.
Device tensors only: there is no CPU path.
"""
from __future__ import annotations

import dataclasses
import os
import warnings
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from .ops import _contig, _ptr, _require_device, _stream

_DT = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}
MAX_L, MAX_K, MAX_TOPK = 256, 64, 256


def _code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {dtype}: float32 (parity), bfloat16 or float16")


def _is_int(t, dim: Optional[int] = None) -> bool:
    """An integer tensor (not float, complex, bool), of ``dim`` dimensions if given."""
    return isinstance(t, Tensor) and not (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool) \
        and (dim is None or t.dim() == dim)


def _is_list(s, i, g=None) -> bool:
    """Scores [U,k] and integer ids [U,k] (and integer interests [U,k], if given) of one shape."""
    return isinstance(s, Tensor) and s.dim() == 2 and _is_int(i, 2) and i.shape == s.shape \
        and (g is None or (_is_int(g, 2) and g.shape == s.shape))


def _cap(cap, what: str) -> int:
    if isinstance(cap, bool) or not isinstance(cap, int) or not 1 <= cap <= MAX_TOPK:
        raise ValueError(f"{what} must be an int in [1, {MAX_TOPK}]")
    return cap


@dataclasses.dataclass
class EncoderWeights:
    """miner_encoder_pack() output."""
    buf: Tensor
    dtype: torch.dtype
    d: int
    Dc: int
    K: int
    has_target: bool


def pack_encoder(w_poly: Tensor, context_codes: Tensor, w_target: Optional[Tensor] = None,
                 dtype: Optional[torch.dtype] = None) -> EncoderWeights:
    """poly_attn.linear.weight [Dc,d], poly_attn.context_codes [K,Dc], target_aware_attn.linear.weight
    [d,d] (model.py:155-157, :198) -> the user encoder's packed layout (K <= 64, Dc <= 256)."""
    _require_device(w_poly, context_codes, w_target)
    dtype = dtype or w_poly.dtype
    dt = _code(dtype)
    w1, q, w2 = _contig(w_poly, dtype), _contig(context_codes, dtype), _contig(w_target, dtype)
    Dc, d = w1.shape
    K = q.shape[0]
    if q.shape[1] != Dc or (w2 is not None and tuple(w2.shape) != (d, d)):
        raise ValueError("weight shapes do not match (w_poly [Dc,d], context_codes [K,Dc], w_target [d,d])")
    nbytes = _lib.lib().miner_encoder_packed_bytes(dt, d, Dc, K)
    if nbytes == 0:
        raise ValueError(f"d={d} Dc={Dc} K={K} not supported (K <= 64, Dc <= 256, d <= 768, d % 64 == 0)")
    buf = torch.empty(nbytes, dtype=torch.uint8, device=w1.device)
    with torch.cuda.device(w1.device):
        rc = _lib.lib().miner_encoder_pack(_stream(w1.device), dt, _ptr(w1), _ptr(q), _ptr(w2), d, Dc, K, _ptr(buf))
    _lib.check(rc, "miner_encoder_pack")
    return EncoderWeights(buf, dtype, d, Dc, K, w2 is not None)


def encode_users(history: Tensor, his_mask: Tensor, packed: EncoderWeights, *, his_ids: Optional[Tensor] = None,
                 his_bias: Optional[Tensor] = None, with_proj: bool = True, return_f32: bool = False):
    """PolyAttention (model.py:159-185) per user, and proj = gelu(mui · W2ᵀ) (model.py:212).

    history [U,L,d] (dense), or the news table [n_news,d] with his_ids [U,L]; his_mask [U,L] bool;
    his_bias [U,L] fp32 or None. Returns (mui, proj) in the packed dtype ([U,K,d]; proj None when
    with_proj is False), plus mui in fp32 when return_f32.
    """
    _require_device(history, his_mask, his_ids, his_bias)
    dt = _code(packed.dtype)
    src = _contig(history, packed.dtype)
    mask = _contig(his_mask, torch.bool).view(torch.uint8)
    U, L = mask.shape
    d, K = packed.d, packed.K
    ids = None
    n_news = 0
    if his_ids is not None:
        ids = _contig(his_ids, torch.int32)
        n_news = src.shape[0]
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n_news):
            raise IndexError(f"his_ids out of range [0, {n_news})")
    elif tuple(src.shape) != (U, L, d):
        raise ValueError(f"history must be [{U},{L},{d}]")
    if not 1 <= L <= MAX_L:
        raise ValueError(f"history length {L} outside [1, {MAX_L}]")
    if with_proj and not packed.has_target:
        raise ValueError("the packed weights hold no w_target: pass with_proj=False")
    bias = _contig(his_bias, torch.float32)
    dev = src.device
    mui = torch.empty(U, K, d, dtype=packed.dtype, device=dev)
    proj = torch.empty(U, K, d, dtype=packed.dtype, device=dev) if with_proj else None
    m32 = torch.empty(U, K, d, dtype=torch.float32, device=dev) if return_f32 else None
    with torch.cuda.device(dev):
        rc = _lib.lib().miner_encode_users(_stream(dev), dt, _ptr(src), _ptr(ids), n_news, _ptr(mask), _ptr(bias),
                                           _ptr(packed.buf), U, L, d, packed.Dc, K, _ptr(m32), _ptr(mui), _ptr(proj))
    _lib.check(rc, "miner_encode_users")
    return (mui, proj, m32) if return_f32 else (mui, proj)


def _pack_bits(mask: Tensor) -> Tensor:
    """bool [N] -> int32 [ceil(N/32)]: news n is bit n & 31 (bit 0 least significant) of word n >> 5."""
    n = mask.shape[0]
    words = (n + 31) // 32
    m = torch.zeros(words * 32, dtype=torch.int64, device=mask.device)
    m[:n] = mask
    w = (m.view(words, 32) << torch.arange(32, dtype=torch.int64, device=mask.device)).sum(dim=1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def pack_eligible(mask: Tensor) -> Tensor:
    """The ranker's eligibility bitmap (include/miner_corpus.h, news_ok) of a bool [N] device tensor:
    int32 [ceil(N/32)], news n at bit n & 31 of word n >> 5."""
    _require_device(mask)
    if mask.dtype != torch.bool or mask.dim() != 1:
        raise ValueError("eligible mask must be a bool [N] tensor")
    return _pack_bits(mask)


def _is_mask(eligible, N: int) -> bool:
    """eligible= for a table of N news: True for a bool [N] mask, False for pack_eligible's int32
    words; anything else is an argument error."""
    words = (N + 31) // 32
    if isinstance(eligible, Tensor) and eligible.dim() == 1:
        if eligible.dtype == torch.bool and eligible.shape[0] == N:
            return True
        if eligible.dtype == torch.int32 and eligible.shape[0] == words:
            return False
    raise ValueError(f"eligible must be bool [{N}] or packed int32 [{words}] (pack_eligible)")


def _eligible_words(eligible: Tensor, N: int) -> Tensor:
    return pack_eligible(eligible) if _is_mask(eligible, N) else eligible.contiguous()


@dataclasses.dataclass
class NewsIdList:
    """canonical_news_ids() output: ids int32 [M] on the device, ascending and distinct, all inside
    [0, N) — the precondition of miner_rank_topk_subset."""
    ids: Tensor
    N: int


def canonical_news_ids(news_ids: Tensor, N: int) -> NewsIdList:
    """Any 1-D integer device tensor of news ids -> the ranker's id list for a table of N news: ids
    outside [0, N) dropped, sorted, repeats removed (on the device). rank_topk / rank_corpus /
    update_topk do this themselves; pass the result instead of the tensor to do it once."""
    _require_device(news_ids)
    if not _is_int(news_ids, 1):
        raise ValueError("news_ids must be a 1-D integer tensor")
    ids = news_ids.to(torch.int64)
    ids = torch.unique(ids[(ids >= 0) & (ids < N)], sorted=True)
    return NewsIdList(ids.to(torch.int32).contiguous(), N)


@dataclasses.dataclass
class _Prior:
    """A checked score prior: bias fp32 [G, N] contiguous on the device, group int32 [U] or None
    (every user reads row 0)."""
    bias: Tensor
    group: Optional[Tensor]

    @property
    def G(self) -> int:
        return self.bias.shape[0]

    def users(self, u0: int, u1: int) -> "_Prior":
        return _Prior(self.bias, None if self.group is None else self.group[u0:u1])


def _prior(news_bias, user_group, U: int, N: int) -> Optional[_Prior]:
    """news_bias= / user_group= of the ranking entries -> a _Prior, or None without a prior. Shapes,
    dtypes and the group values are checked; that the tensors are on the device is the caller's check."""
    if news_bias is None:
        if user_group is not None:
            raise ValueError("user_group without news_bias")
        return None
    if not isinstance(news_bias, Tensor) or news_bias.dtype != torch.float32 or news_bias.dim() not in (1, 2) \
            or news_bias.shape[-1] != N or news_bias.shape[0] < 1:
        raise ValueError(f"news_bias must be a float32 [{N}] or [G, {N}] tensor")
    G = 1 if news_bias.dim() == 1 else news_bias.shape[0]
    if user_group is None:
        if G > 1:
            raise ValueError(f"news_bias holds {G} rows: user_group [{U}] says which row a user reads")
    else:
        if not _is_int(user_group, 1) or user_group.shape[0] != U:
            raise ValueError(f"user_group must be an integer [{U}] tensor")
        if U and (int(user_group.min()) < 0 or int(user_group.max()) >= G):
            raise ValueError(f"user_group out of range [0, {G})")
    return _Prior(news_bias.reshape(G, N).contiguous(), _contig(user_group, torch.int32))


def _prior_args(pri: Optional[_Prior]):
    """(news_bias, G, user_group) of the C entries: a checked prior's, or NULL / 0 / NULL without one."""
    return (None, 0, None) if pri is None else (_ptr(pri.bias), pri.G, _ptr(pri.group))


@dataclasses.dataclass
class _Caps:
    """Checked per-cluster caps: cluster int32 [N] contiguous on the device, cap in [1, MAX_TOPK]."""
    cluster: Tensor
    cap: int


def _caps(news_cluster, cluster_cap, N: Optional[int]) -> Optional[_Caps]:
    """news_cluster= / cluster_cap= of the ranking and merging entries -> a _Caps, or None without
    caps; that the table is on the device is the caller's check. ``N``: the length the table must
    have (None: any, at least one entry — the merging entries)."""
    if news_cluster is None and cluster_cap is None:
        return None
    if news_cluster is None or cluster_cap is None:
        raise ValueError("news_cluster and cluster_cap go together")
    _cap(cluster_cap, "cluster_cap")
    if not _is_int(news_cluster, 1) or news_cluster.shape[0] < 1 or (N is not None and news_cluster.shape[0] != N):
        raise ValueError("news_cluster must be a 1-D integer tensor" + (f" of {N} entries" if N is not None else ""))
    if news_cluster.dtype != torch.int32:
        if int(news_cluster.min()) < -2 ** 31 or int(news_cluster.max()) > 2 ** 31 - 1:
            raise ValueError("news_cluster values must fit int32")
    return _Caps(_contig(news_cluster, torch.int32), cluster_cap)


@dataclasses.dataclass
class _Cursor:
    """Checked keyset cursors: scores fp32 [U] and ids int32 [U], contiguous on the device."""
    scores: Tensor
    ids: Tensor

    def users(self, u0: int, u1: int) -> "_Cursor":
        return _Cursor(self.scores[u0:u1], self.ids[u0:u1])


_INT32_MAX = 2 ** 31 - 1


def _cursor(after, U: int) -> Optional[_Cursor]:
    """after= of the ranking entries -> a _Cursor, or None without one. Shapes and dtypes are checked
    (that the pair is on the device is the caller's check); ids of a dtype wider than int32 must fit int32."""
    if after is None:
        return None
    try:
        s, i = after
    except (TypeError, ValueError):
        raise ValueError("after must be a (scores, ids) pair")
    if not isinstance(s, Tensor) or s.dtype != torch.float32 or s.dim() != 1 or s.shape[0] != U:
        raise ValueError(f"after: the scores must be a float32 [{U}] tensor")
    if not _is_int(i, 1) or i.shape[0] != U:
        raise ValueError(f"after: the ids must be an integer [{U}] tensor")
    if i.dtype not in (torch.int32, torch.int16, torch.int8, torch.uint8) and U:
        if int(i.min()) < -2 ** 31 or int(i.max()) > _INT32_MAX:
            raise ValueError("after: the ids must fit int32")
    return _Cursor(s.contiguous(), _contig(i, torch.int32))


def start_cursor(U: int, device):
    """The cursor before everything, (+inf, -1) for each of U users: rank_topk(after=start_cursor(...))
    is the first page — the list of the call without a cursor."""
    return (torch.full((U,), float("inf"), dtype=torch.float32, device=device),
            torch.full((U,), -1, dtype=torch.int32, device=device))


def page_cursor(lists):
    """The cursor that continues ``lists`` = (scores [U,k], ids [U,k]), a page rank_topk returned:
    per row its last entry if the row is full, else (-inf, 2^31 - 1), "after everything" — a short
    row means the ranking ended. (Not the (-inf, -1) tail itself: a cursor there would list the news
    that score -inf once more.) Pure tensor operations on the lists' device, no host synchronisation."""
    try:
        s, i = lists
    except (TypeError, ValueError):
        raise ValueError("lists must be a (scores, ids) pair")
    if not _is_list(s, i) or s.shape[1] < 1 or not s.is_floating_point():
        raise ValueError("lists: scores [U,k] and integer ids [U,k] of one shape, k >= 1")
    last_s, last_i = s[:, -1].to(torch.float32), i[:, -1]
    full = last_i >= 0
    return (torch.where(full, last_s, float("-inf")).contiguous(),
            torch.where(full, last_i, _INT32_MAX).to(torch.int32).contiguous())


MAX_WALK_GROUPS = 1024


@dataclasses.dataclass
class WalkState:
    """The state of a capped walk between two pages (include/miner_corpus.h, miner_rank_topk_resume):
    per user the keyset cursor — scores fp32 [U], ids int32 [U] — and the table of the groups served so
    far: groups / counts int32 [U, Q] (the first n_used[u] pairs of row u, groups strictly ascending
    and >= 0: cluster ids under news_cluster, interests under interest_cap), n_used int32 [U], and
    overflow uint8 [U] (1: the user needed more than Q distinct groups and its walk was ended — its
    cursor is "after everything" — rather than a cap ever broken). start_walk makes the first,
    advance_walk the next; a hand-made one must keep the table sorted."""
    scores: Tensor
    ids: Tensor
    groups: Tensor
    counts: Tensor
    n_used: Tensor
    overflow: Tensor

    @property
    def cursor(self):
        return self.scores, self.ids

    @property
    def capacity(self) -> int:
        return self.groups.shape[1]

    def users(self, u0: int, u1: int) -> "WalkState":
        return WalkState(self.scores[u0:u1], self.ids[u0:u1], self.groups[u0:u1], self.counts[u0:u1], self.n_used[u0:u1],
                         self.overflow[u0:u1])


def _walk_state(state, U: Optional[int]) -> WalkState:
    """resume= / advance_walk's state -> a checked WalkState with contiguous fields. Types, dtypes and
    shapes are checked; that the fields are on the device is the caller's check."""
    if not isinstance(state, WalkState):
        raise ValueError("resume must be a WalkState (start_walk, advance_walk)")
    fields = (state.scores, state.ids, state.groups, state.counts, state.n_used, state.overflow)
    if not all(isinstance(t, Tensor) for t in fields):
        raise ValueError("WalkState: every field is a tensor")
    n = state.scores.shape[0] if state.scores.dim() == 1 else -1
    if U is not None and n != U:
        raise ValueError(f"the walk state was made for {n} users, not {U}")
    if state.scores.dtype != torch.float32 or state.scores.dim() != 1 or state.ids.dtype != torch.int32 \
            or tuple(state.ids.shape) != (n,):
        raise ValueError(f"WalkState: the cursor is scores float32 [{n}] and ids int32 [{n}]")
    if state.groups.dtype != torch.int32 or state.counts.dtype != torch.int32 or state.groups.dim() != 2 \
            or state.groups.shape[0] != n or state.counts.shape != state.groups.shape \
            or state.groups.shape[1] > MAX_WALK_GROUPS:
        raise ValueError(f"WalkState: groups and counts are int32 [{n}, Q] of one shape, Q <= {MAX_WALK_GROUPS}")
    if state.n_used.dtype != torch.int32 or tuple(state.n_used.shape) != (n,) or state.overflow.dtype != torch.uint8 \
            or tuple(state.overflow.shape) != (n,):
        raise ValueError(f"WalkState: n_used is int32 [{n}] and overflow uint8 [{n}]")
    return WalkState(*(t.contiguous() for t in fields))


def _capacity(capacity) -> int:
    if isinstance(capacity, bool) or not isinstance(capacity, int) or not 0 <= capacity <= MAX_WALK_GROUPS:
        raise ValueError(f"capacity must be an int in [0, {MAX_WALK_GROUPS}]")
    return capacity


def start_walk(U: int, device, capacity: int = MAX_WALK_GROUPS) -> WalkState:
    """The state before everything: the cursor (+inf, -1) and an empty table with room for
    ``capacity`` distinct groups per user (at most 1,024). rank_topk(..., resume=start_walk(...)) is
    the first page — the capped list of the call without ``resume``, bit for bit."""
    Q = _capacity(capacity)
    s, i = start_cursor(U, device)
    return WalkState(s, i, torch.zeros(U, Q, dtype=torch.int32, device=device),
                     torch.zeros(U, Q, dtype=torch.int32, device=device), torch.zeros(U, dtype=torch.int32, device=device),
                     torch.zeros(U, dtype=torch.uint8, device=device))


def advance_walk(state: WalkState, page, *, news_cluster=None) -> WalkState:
    """The state after ``page`` was served from ``state`` (miner_walk_advance: one small launch, no
    host synchronisation): the page's page_cursor, and the state's table plus the groups of the page's
    entries — a (scores, ids) pair under ``news_cluster`` (the integer table; an id at or past its
    length has no group), or a (scores, ids, interests) triple without it,
    as rank_topk(interest_cap=, return_interest=True) returns. Tail entries and entries in no group
    add nothing. The new state has the old one's capacity; a user that would need more distinct
    groups gets overflow 1 and the cursor "after everything" (its next page is empty), and an
    overflow stays set in the states that follow. The arguments are checked before anything touches
    the device; the outputs are new tensors."""
    triple = _is_triple(page)
    if triple == (news_cluster is not None):
        raise ValueError("advance_walk: a (scores, ids) page with news_cluster, or a (scores, ids, interests) page without")
    st = _walk_state(state, None)
    U = st.groups.shape[0]
    try:
        ps, pi, pg = page if triple else (*page, None)
    except (TypeError, ValueError):
        raise ValueError("page must be a (scores, ids) pair or a (scores, ids, interests) triple")
    if not _is_list(ps, pi) or not ps.is_floating_point() or ps.shape[0] != U or not 1 <= ps.shape[1] <= MAX_TOPK:
        raise ValueError(f"page: scores [{U},k] and integer ids [{U},k] of one shape, 1 <= k <= {MAX_TOPK}")
    if triple and not _is_list(ps, pi, pg):
        raise ValueError("page: integer interests of the page's shape [U,k]")
    clus = None if triple else _caps(news_cluster, 1, None).cluster
    _require_device(ps, pi, pg, clus, *vars(st).values())
    return _advance(st, _contig(ps, torch.float32), _contig(pi, torch.int32), _contig(pg, torch.int32), clus)


def _advance(st: WalkState, ps: Tensor, pi: Tensor, pg: Optional[Tensor], clus: Optional[Tensor]) -> WalkState:
    """advance_walk on checked arguments: the page fp32 / int32 [U,k] contiguous, its groups the
    interests ``pg``, or else the clusters of the int32 table ``clus``."""
    U, Q = st.groups.shape
    dev = ps.device
    k = ps.shape[1]
    out = WalkState(torch.empty(U, dtype=torch.float32, device=dev), torch.empty(U, dtype=torch.int32, device=dev),
                    torch.zeros(U, Q, dtype=torch.int32, device=dev), torch.zeros(U, Q, dtype=torch.int32, device=dev),
                    torch.empty(U, dtype=torch.int32, device=dev), torch.empty(U, dtype=torch.uint8, device=dev))
    with torch.cuda.device(dev):
        rc = _lib.lib().miner_walk_advance(_stream(dev), _ptr(ps), _ptr(pi), _ptr(pg), _ptr(clus),
                                           0 if clus is None else clus.shape[0], _ptr(st.groups) if Q else None,
                                           _ptr(st.counts) if Q else None, _ptr(st.n_used), Q, _ptr(out.scores), _ptr(out.ids),
                                           _ptr(out.groups) if Q else None, _ptr(out.counts) if Q else None, _ptr(out.n_used),
                                           _ptr(out.overflow), U, k, Q)
    _lib.check(rc, "miner_walk_advance")
    out.overflow |= st.overflow
    return out


def _dominant_interest(score_type: str) -> None:
    if score_type == "mean":
        raise ValueError("score_type 'mean' has no dominant interest: interest_cap / return_interest need 'weighted' or 'max'")


@dataclasses.dataclass(slots=True)      # (built on every call: the slots make that cheaper)
class _Request:
    """Everything a ranking call takes besides the user vectors, the table and topk — checked,
    converted and on the device: the exclusions int32 [U,E] (None: none), the eligibility words, the
    id list, the prior, the caps, the cursor and the walk state (a walk carries its own cursor),
    icap (0: no per-interest cap), return_interest and the score type."""
    excl: Optional[Tensor]
    ok: Optional[Tensor]
    sub: Optional[NewsIdList]
    prior: Optional[_Prior]
    caps: Optional[_Caps]
    cursor: Optional[_Cursor]
    walk: Optional[WalkState]
    icap: int
    return_interest: bool
    score_type: str

    def users(self, u0: int, u1: int) -> "_Request":
        """The request of the users [u0, u1): what is per user is sliced, the rest shared."""
        def cut(x):
            return None if x is None else x[u0:u1] if isinstance(x, Tensor) else x.users(u0, u1)
        # (once per batch: built directly, dataclasses.replace costs several times as much)
        return _Request(cut(self.excl), self.ok, self.sub, cut(self.prior), self.caps, cut(self.cursor), cut(self.walk),
                        self.icap, self.return_interest, self.score_type)


def _request(U: int, N: int, *, score_type: str = "weighted", exclude_ids=None, eligible=None, news_ids=None,
             news_bias=None, user_group=None, news_cluster=None, cluster_cap=None, after=None, interest_cap=None,
             return_interest: bool = False, resume=None) -> _Request:
    """The keyword options of the ranking entries, for U users and a table of N news -> a _Request.
    The one place the options' combination rules live. Every argument error is raised before the
    device check; the bitmap is packed and the id list canonicalised after it, once."""
    capped = news_cluster is not None or cluster_cap is not None
    icap = 0
    if interest_cap is not None or return_interest:
        _dominant_interest(score_type)
    if interest_cap is not None:
        # the capped form's restrictions: one group per entry in the ranker's merge, and no cursor
        icap = _cap(interest_cap, "interest_cap")
        if capped:
            raise ValueError("interest_cap cannot be combined with news_cluster / cluster_cap")
        if after is not None:
            raise ValueError("interest_cap cannot be combined with after= (there is no cursor under caps)")
    if after is not None and capped:
        # a capped walk also needs the earlier pages' per-cluster counts, which a (score, id) pair does not carry
        raise ValueError("after= cannot be combined with news_cluster / cluster_cap")
    if resume is not None and after is not None:
        raise ValueError("resume= carries its own cursor: it cannot be combined with after=")
    if resume is not None and not capped and not icap:
        raise ValueError("resume= continues a capped list: it needs news_cluster / cluster_cap or interest_cap")
    walk = None if resume is None else _walk_state(resume, U)
    # (a checker is called only where its option is given: the plain call pays for none of them)
    prior = None if news_bias is None and user_group is None else _prior(news_bias, user_group, U, N)
    caps = _caps(news_cluster, cluster_cap, N) if capped else None
    cursor = None if after is None else _cursor(after, U)
    E = 0
    if exclude_ids is not None:
        if not _is_int(exclude_ids, 2) or exclude_ids.shape[0] != U:
            raise ValueError(f"exclude_ids must be an integer [{U}, E] tensor")
        E = exclude_ids.shape[1]
        if E > MAX_L:
            raise ValueError(f"exclude_ids holds {E} ids per user, more than {MAX_L}")
    mask = eligible is not None and _is_mask(eligible, N)
    listed = isinstance(news_ids, NewsIdList)
    if listed and news_ids.N != N:
        raise ValueError(f"the id list was made for a table of {news_ids.N} news, not {N}")
    if news_ids is not None and not listed and not _is_int(news_ids, 1):
        raise ValueError("news_ids must be a 1-D integer tensor")
    _require_device(exclude_ids, eligible, news_ids.ids if listed else news_ids,
                    *[t for x in (prior, caps, cursor, walk) if x is not None for t in vars(x).values()])
    excl = ok = sub = None
    if E:
        excl = _contig(exclude_ids, torch.int32)
    if eligible is not None:
        ok = pack_eligible(eligible) if mask else eligible.contiguous()
    if news_ids is not None:
        sub = news_ids if listed else canonical_news_ids(news_ids, N)
    return _Request(excl, ok, sub, prior, caps, cursor, walk, icap, return_interest, score_type)


def _rank(mui: Tensor, proj: Optional[Tensor], tab: Tensor, topk: int, req: _Request):
    """One ranked page for _rank_operands' user vectors and table under a request: (scores, ids), or
    (scores, ids, interests) with req.return_interest. The one caller of the library's ranking entry
    — the widest, miner_rank_topk_resume: what the request does not hold is NULL and launches the
    narrower entry's kernel. Called by the public entries themselves (the warning's stack level)."""
    U, K, d = mui.shape
    N = tab.shape[0]
    if not 1 <= topk <= MAX_TOPK:
        raise ValueError(f"topk must be in [1, {MAX_TOPK}]")
    icap, caps, walk, sub = req.icap, req.caps, req.walk, req.sub
    if icap and topk > icap * K:
        # the result is right, the step is slow (see rank_topk's docstring): say so once per call site
        warnings.warn(f"rank_topk: topk={topk} exceeds interest_cap * K = {icap * K}: the list can never fill, so every "
                      f"step merges all its news (several times the capped step); ask for topk <= {icap * K}",
                      RuntimeWarning, stacklevel=3)
    st, dt = _lib.SCORE_TYPES[req.score_type], _DT[mui.dtype]
    dev = mui.device
    top_s = torch.empty(U, topk, dtype=torch.float32, device=dev)
    top_i = torch.empty(U, topk, dtype=torch.int32, device=dev)
    top_g = torch.empty(U, topk, dtype=torch.int32, device=dev) if icap and req.return_interest else None
    # a workspace only where the split form runs: the library's recommendation (U <= 510 on a 256-CU
    # device), or MINER_RK_SPLIT=1 / 0 (read here, per call: a test / A/B switch) forcing either form
    lib = _lib.lib()
    force = os.environ.get("MINER_RK_SPLIT", "")
    split = force == "1" if force in ("0", "1") else bool(lib.miner_rank_topk_split_recommended(U))
    split = split and caps is None and icap == 0
    nws = int(lib.miner_rank_topk_workspace_bytes(U, topk)) if split else 0
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
    M = -1 if sub is None else sub.ids.numel()               # -1 with no list: the whole table
    cur = req.cursor if walk is None else walk               # a walk carries its own cursor
    # the served-group table: all NULL and Q = 0 without a walk (an empty [U, 0] table has no storage:
    # any aligned non-NULL address stands for it, never read)
    Q = 0 if walk is None else walk.capacity
    used = (None, None, None) if walk is None else \
        (_ptr(walk.groups if Q else walk.n_used), _ptr(walk.counts if Q else walk.n_used), _ptr(walk.n_used))
    with torch.cuda.device(dev):
        rc = lib.miner_rank_topk_resume(
            _stream(dev), dt, st, _ptr(mui), _ptr(proj), _ptr(tab), U, N, d, K, topk,
            _ptr(req.excl), 0 if req.excl is None else req.excl.shape[1], _ptr(req.ok),
            _ptr(sub.ids) if M > 0 else None, M, _ptr(top_s), _ptr(top_i), _ptr(ws), nws, *_prior_args(req.prior),
            None if caps is None else _ptr(caps.cluster), 0 if caps is None else caps.cap,
            None if cur is None else _ptr(cur.scores), None if cur is None else _ptr(cur.ids), icap, _ptr(top_g), *used, Q)
    _lib.check(rc, "miner_rank_topk")
    if not req.return_interest:
        return top_s, top_i
    if top_g is None:        # no cap: the pair form on the listed ids (a tail id of -1 gives -1)
        top_g = _score_pairs(st, dt, mui, proj, tab, top_i.to(torch.int64), None, True)[1]
    return top_s, top_i, top_g


def rank_topk(user_mui: Tensor, user_proj: Optional[Tensor], news: Tensor, topk: int, *,
              score_type: str = "weighted", exclude_ids: Optional[Tensor] = None,
              eligible: Optional[Tensor] = None, news_ids=None, news_bias=None,
              user_group: Optional[Tensor] = None, news_cluster=None, cluster_cap: Optional[int] = None,
              after=None, interest_cap: Optional[int] = None, return_interest: bool = False, resume=None):
    """Top-k news per user by the click score, best first: (scores [U,topk] fp32, ids [U,topk]
    int32); entries past the table size are (-inf, -1).

    exclude_ids [U,E] (any integer dtype, E <= 256): news ids kept out of user u's list; entries
    outside [0, N), such as a -1 padding, exclude nothing. eligible: bool [N], or the packed int32
    [ceil(N/32)] of pack_eligible: only these news are ranked. A list with fewer survivors than
    topk ends in (-inf, -1) entries; the scores themselves never change.

    news_ids: a 1-D integer tensor (any order, repeats and ids outside [0, N) allowed) or a
    canonical_news_ids() list: only these table rows are read and ranked, so the time follows their
    count M, not N. The list is, bit for bit, that of ``eligible`` = "n is in news_ids" (with
    ``eligible`` given too: the intersection), which streams the whole table whatever it holds.
    Measured on 2,048 users x 200,000 news (fp16, K = 64, d = 768, profiles/rk_subset_ab.txt): 1 % of
    the table 0.021x, 5 % 0.064x, 25 % 0.270x, 100 % 1.024x the bitmap form's 78 ms — the bitmap form
    is the faster one only above M/N of about 0.98. Nothing reroutes an ``eligible=`` call: the caller chooses the form.

    news_bias: a score prior, float32 [N] or [G, N] on the device (recency, popularity, an editorial
    boost, a per-edition weight), with user_group an integer [U] tensor of rows in [0, G) (required
    when G > 1). The list is ranked by fp32(score + news_bias[user_group[u], n]) — one IEEE add on the
    unbiased score, so ``scores + prior`` in torch fp32 reproduces it bit for bit — and that sum is
    the score returned. Filters, ties (lower id first) and ``news_ids`` work on the table id as
    before. A prior is not a filter: a -inf prior still lists the news while a list has room (use
    ``eligible``); +inf ranks it first; a NaN sum is never listed. Without news_bias the call is
    today's.

    news_cluster / cluster_cap: per-cluster caps. news_cluster is an integer [N] tensor (values must
    fit int32): >= 0 the cluster of news n (a story, a publisher; arbitrary values), < 0 in no
    cluster; cluster_cap an int in [1, 256]; one without the other is an error. The list is the walk
    of the user's complete ranking (under every other argument, as with topk = N) that keeps an entry
    iff fewer than cluster_cap entries of its cluster were kept before it, stopped after topk kept
    entries ((-inf, -1) after a shorter one). Scores are the uncapped call's, bit for bit; an
    excluded or ineligible news uses up no cap. The capped ranker has no split form: a batch of
    U <= 510 users runs the unsplit kernel (MINER_RK_SPLIT is ignored), at the price
    profiles/rk_cap_ab.txt records. With both None the call is today's.

    after: a keyset cursor, (scores [U] float32, ids [U] integer) on the device — start_cursor,
    page_cursor of an earlier page, or any pair. The list then holds the first topk entries of the
    user's ranking (score descending, then lower id; under every other argument) that come strictly
    after (scores[u], ids[u]): a lower score, or an equal one (a float compare: -0 equals +0) with a
    higher id. The score compared is the one ranked (the biased sum under a prior), the id the table
    id. Listed scores are those of the call without a cursor, bit for bit, and the pages chained with
    page_cursor are disjoint and concatenate to the complete ranking. (+inf, -1) is before
    everything, (-inf, 2^31 - 1) after everything, a NaN score lists nothing, and the cursor need not
    be a listed, eligible or existing news: it is a position in the order. Each page streams the
    table once (the price: profiles/rk_after_ab.txt). A cursor alone does not continue a capped list
    (a capped walk also needs the earlier pages' per-cluster counts): ``after`` with news_cluster /
    cluster_cap raises ValueError — ``resume`` is the way. Without ``after`` the call is today's.

    resume: a WalkState (start_walk, advance_walk) — the cursor under caps. With news_cluster /
    cluster_cap or interest_cap (one of them; without a cap, or together with ``after``: ValueError) the
    list is the capped walk continued strictly after the state's cursor, in which a group g already
    has state.counts' used(g) entries: an entry is kept iff it is in no group or used(g) + (entries of
    g kept earlier in this call) < cap. Scores are the uncapped call's, bit for bit, and the pages
    chained with advance_walk concatenate to the capped walk of any depth — also when the cap or topk
    change between pages. resume=start_walk(...) is the call without it, bit for bit.
    ``return_interest`` works as under interest_cap. The unsplit kernel, as every capped call; the
    price: profiles/rk_resume_ab.txt. Without ``resume`` the call is today's.

    return_interest: the call returns (scores, ids, interests): interests int32 [U,topk], the
    dominant interest of each listed pair — the lowest k in [0, K) whose value equals the maximum
    the score's own reduction over K found ('weighted': the largest target-aware softmax weight,
    model.py:213; 'max': the arg-max of M_k, model.py:129), -1 in the tail. Without interest_cap it is
    the call without it followed by score_pairs(return_interest=True) on the returned ids: the list
    is bit for bit the plain call's and no other ranking kernel runs.

    interest_cap: an int in [1, 256]: at most interest_cap news of one dominant interest in a user's
    list — the capped walk above with the pair's interest in place of the news's cluster (for one
    user: news_cluster = that user's interests, which no table can say for several). Scores are the
    uncapped call's, bit for bit. As the per-cluster caps: the unsplit kernel, no ``after``, and not
    together with news_cluster / cluster_cap (ValueError). 'mean' has no dominant interest: either
    argument with it raises ValueError. A list holds at most interest_cap · K entries: a larger topk
    never fills, and a list that never fills merges every news of every step (5.15x the step at
    cap 1, K = 64, topk = 100) — keep topk <= interest_cap · K; a call that does not gets a
    RuntimeWarning (the list is still exact: the kernel does not clamp topk, because an entry in no
    group — 'max' over a row whose M_k are all NaN scores -inf with interest -1 — is always kept, so
    a list can hold more than interest_cap · K entries). The price otherwise, 1.01 - 1.03x the
    capped step: profiles/rk_interest_ab.txt. With neither the call is today's."""
    req = _request(user_mui.shape[0], news.shape[0], score_type=score_type, exclude_ids=exclude_ids, eligible=eligible,
                   news_ids=news_ids, news_bias=news_bias, user_group=user_group, news_cluster=news_cluster,
                   cluster_cap=cluster_cap, after=after, interest_cap=interest_cap, return_interest=return_interest,
                   resume=resume)
    _, _, mui, proj, tab = _rank_operands(user_mui, user_proj, news, score_type)
    return _rank(mui, proj, tab, topk, req)


def rank_topk_deep(user_mui: Tensor, user_proj: Optional[Tensor], news: Tensor, topk: int, *, after=None,
                   score_type: str = "weighted", exclude_ids: Optional[Tensor] = None,
                   eligible: Optional[Tensor] = None, news_ids=None, news_bias=None,
                   user_group: Optional[Tensor] = None, news_cluster=None, cluster_cap=None, interest_cap=None,
                   return_interest: bool = False):
    """rank_topk for any topk >= 1: (scores [U,topk] fp32, ids [U,topk] int32), best first, with the
    (-inf, -1) tail — ceil(topk / 256) pages of rank_topk chained with page_cursor (the first from
    ``after``, or from the top without it) and written side by side. Every page streams the table
    once, so the cost is pages x the rank_topk step (profiles/rk_after_ab.txt), not one pass: a deep
    list is paid for by its depth. The other arguments are rank_topk's; ``news_ids`` is canonicalised
    once, the bitmap packed once and the prior checked once. No host synchronisation beyond
    rank_topk's own argument checks. Caps are not offered here (a cursor alone does not continue a
    capped list; rank_topk_deep_capped pages with walk states): ``news_cluster`` / ``cluster_cap`` are
    named only to say so, anything but None raises ValueError; so is ``interest_cap``. ``return_interest`` (per page, as in rank_topk) adds interests [U,topk]
    int32 as a third result."""
    if news_cluster is not None or cluster_cap is not None:
        raise ValueError("rank_topk_deep pages with cursors, and there is no cursor under news_cluster / cluster_cap")
    if interest_cap is not None:
        raise ValueError("rank_topk_deep pages with cursors, and there is no cursor under interest_cap")
    if isinstance(topk, bool) or not isinstance(topk, int) or topk < 1:
        raise ValueError("topk must be an int >= 1")
    U = user_mui.shape[0]
    req = _request(U, news.shape[0], score_type=score_type, exclude_ids=exclude_ids, eligible=eligible, news_ids=news_ids,
                   news_bias=news_bias, user_group=user_group, after=after, return_interest=return_interest)
    _, _, mui, proj, tab = _rank_operands(user_mui, user_proj, news, score_type)
    out = tuple(torch.empty(U, topk, dtype=dt, device=mui.device)
                for dt in (torch.float32, torch.int32, torch.int32)[:3 if return_interest else 2])
    for k0 in range(0, topk, MAX_TOPK):
        k1 = min(topk, k0 + MAX_TOPK)
        page = _rank(mui, proj, tab, k1 - k0, req)
        for dst, src in zip(out, page):
            dst[:, k0:k1] = src
        if k1 < topk:
            req = dataclasses.replace(req, cursor=_Cursor(*page_cursor(page[:2])))
    return out


def rank_topk_deep_capped(user_mui: Tensor, user_proj: Optional[Tensor], news: Tensor, topk: int, *, resume=None,
                          return_state: bool = False, score_type: str = "weighted",
                          exclude_ids: Optional[Tensor] = None, eligible: Optional[Tensor] = None, news_ids=None,
                          news_bias=None, user_group: Optional[Tensor] = None, news_cluster=None, cluster_cap=None,
                          interest_cap=None, return_interest: bool = False, capacity: int = MAX_WALK_GROUPS):
    """The capped rank_topk for any topk >= 1 (news_cluster / cluster_cap, or interest_cap — one of
    them): (scores [U,topk] fp32, ids [U,topk] int32), best first, with the (-inf, -1) tail —
    ceil(topk / 256) resumed pages of rank_topk(resume=) chained with advance_walk on the device (the
    first from ``resume``, or from start_walk(U, device, capacity) without it) and written side by
    side. Every page streams the table once: the cost is pages x the resumed step
    (profiles/rk_resume_ab.txt). The other arguments are rank_topk's; ``news_ids`` is canonicalised
    once, the bitmap packed once, the prior and the caps checked once. No host synchronisation beyond
    rank_topk's own argument checks. ``return_interest`` (under interest_cap) adds interests [U,topk]
    int32 as a third result, ``return_state`` the WalkState after the last page as the last one: one
    more rank_topk(resume=state) continues the walk.
    A walk that starts from the empty state serves at most topk entries and so meets at most topk
    distinct groups: topk <= capacity can never overflow. Beyond that (a deeper cluster-capped list,
    or a ``resume`` state that already holds groups) a user that meets more than ``capacity`` distinct
    groups gets state.overflow = 1 and its list ends there ((-inf, -1) from the next page on) rather
    than a cap ever being broken; under interest_cap there are at most K <= 64 groups."""
    if isinstance(topk, bool) or not isinstance(topk, int) or topk < 1:
        raise ValueError("topk must be an int >= 1")
    U = user_mui.shape[0]
    if news_cluster is None and cluster_cap is None and interest_cap is None:      # (both kinds: _request's error)
        raise ValueError("rank_topk_deep_capped needs news_cluster / cluster_cap or interest_cap (one of them); "
                         "rank_topk_deep is the uncapped deep list")
    if return_interest and interest_cap is None:
        raise ValueError("return_interest: the interests are listed under interest_cap")
    Q = _capacity(capacity)
    # (under interest_cap every page lists its interests: they are the groups advance_walk counts)
    req = _request(U, news.shape[0], score_type=score_type, exclude_ids=exclude_ids, eligible=eligible, news_ids=news_ids,
                   news_bias=news_bias, user_group=user_group, news_cluster=news_cluster, cluster_cap=cluster_cap,
                   interest_cap=interest_cap, return_interest=interest_cap is not None, resume=resume)
    _, _, mui, proj, tab = _rank_operands(user_mui, user_proj, news, score_type)
    if req.walk is None:
        req = dataclasses.replace(req, walk=start_walk(U, mui.device, Q))
    clus = None if req.caps is None else req.caps.cluster
    out = tuple(torch.empty(U, topk, dtype=dt, device=mui.device)
                for dt in (torch.float32, torch.int32, torch.int32)[:3 if return_interest else 2])
    for k0 in range(0, topk, MAX_TOPK):
        k1 = min(topk, k0 + MAX_TOPK)
        page = _rank(mui, proj, tab, k1 - k0, req)
        for dst, src in zip(out, page):
            dst[:, k0:k1] = src
        if k1 < topk or return_state:
            req = dataclasses.replace(req, walk=_advance(req.walk, page[0], page[1], None if req.caps else page[2], clus))
    return out + (req.walk,) if return_state else out


def _list_pair(lists, what: str):
    """(scores, ids) -> the checked pair, fp32 and int32 [U,k]; that it is on the device is the caller's check."""
    try:
        s, i = lists
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a (scores, ids) pair")
    if not _is_list(s, i):
        raise ValueError(f"{what}: scores [U,k] and integer ids [U,k] of one shape")
    if s.shape[1] > MAX_TOPK:
        raise ValueError(f"{what} is {s.shape[1]} wide, more than {MAX_TOPK}")
    return _contig(s, torch.float32), _contig(i, torch.int32)


def _is_triple(lists) -> bool:
    return isinstance(lists, (tuple, list)) and len(lists) == 3


def _list_triple(lists, what: str):
    """(scores, ids, interests) -> the checked pair plus the interests int32 [U,k]."""
    g = lists[2]
    if not _is_int(g) or not isinstance(lists[0], Tensor) or g.shape != lists[0].shape:
        raise ValueError(f"{what}: integer interests of the lists' shape [U,k]")
    return *_list_pair(lists[:2], what), _contig(g, torch.int32)


def merge_topk(a, b, topk: Optional[int] = None, *, eligible: Optional[Tensor] = None, news_cluster=None,
               cluster_cap: Optional[int] = None, interest_cap: Optional[int] = None):
    """Merge two per-user top-k lists (scores [U,k] fp32, ids [U,k] integer; k <= 256 each) on the
    device under the ranker's order (score descending, then lower news id): the best ``topk``
    (default: the wider list's k) of their union, then the (-inf, -1) tail. A news in both lists
    keeps b's entry — a fresh score replaces a stale one — and entries with id < 0 hold nothing; the
    rows need not be sorted. ``eligible`` (bool [N] or pack_eligible's int32 words; a bool mask gives
    N, packed words cover 32 · len news) drops the entries of news that are no longer eligible.
    For disjoint id sets A and B, merge_topk(rank(A), rank(B)) is rank(A ∪ B), bit for bit.
    ``news_cluster`` / ``cluster_cap`` (as in rank_topk; the table may be any length >= 1, an id at or
    past it is in no cluster): after the replacement and the pruning, the capped walk over what is
    left — the inputs need not be capped. Capped lists merge as top-k lists do: for disjoint A and
    B, merge_topk(capped(A), capped(B), caps) is capped(A ∪ B), bit for bit.
    With (scores, ids, interests) triples (rank_topk's ``return_interest``) the result is a triple:
    every entry carries its interest along (b's entry keeps b's), and ``interest_cap`` (an int in
    [1, 256]) runs the capped walk with the entry's own interest as its group — for disjoint A and B
    the interest-capped lists of one user merge to the interest-capped ranking of A ∪ B, bit for
    bit. A pair mixed with a triple, ``interest_cap`` with pairs, and ``interest_cap`` or triples
    together with news_cluster / cluster_cap raise ValueError. There is no ``resume=`` here: the merge
    caps what its two lists hold, counting every group from 0 (a later page of a resumed walk is not
    a capped list on its own, so pages are concatenated, not merged)."""
    triple = _is_triple(a)
    if triple != _is_triple(b):
        raise ValueError("merge_topk: both lists are (scores, ids) pairs or both (scores, ids, interests) triples")
    if interest_cap is not None:
        _cap(interest_cap, "interest_cap")
        if not triple:
            raise ValueError("interest_cap needs (scores, ids, interests) triples")
    if triple and (news_cluster is not None or cluster_cap is not None):
        raise ValueError("lists with interests cannot be merged under news_cluster / cluster_cap")
    caps = _caps(news_cluster, cluster_cap, None)
    _require_device(news_cluster)
    a_g = b_g = None
    if triple:
        a_s, a_i, a_g = _list_triple(a, "list a")
        b_s, b_i, b_g = _list_triple(b, "list b")
    else:
        a_s, a_i = _list_pair(a, "list a")
        b_s, b_i = _list_pair(b, "list b")
    _require_device(a_s, a_i, a_g, b_s, b_i, b_g)
    U, ka = a_s.shape
    kb = b_s.shape[1]
    if b_s.shape[0] != U:
        raise ValueError(f"the lists hold {U} and {b_s.shape[0]} users")
    topk = max(ka, kb) if topk is None else topk
    if not 1 <= topk <= MAX_TOPK:
        raise ValueError(f"topk must be in [1, {MAX_TOPK}]")
    _require_device(eligible)
    ok, N = None, 0
    if eligible is not None:
        if eligible.dim() == 1 and eligible.dtype == torch.bool:
            ok, N = pack_eligible(eligible), eligible.shape[0]
        elif eligible.dim() == 1 and eligible.dtype == torch.int32:
            ok, N = eligible.contiguous(), 32 * eligible.shape[0]
        else:
            raise ValueError("eligible must be bool [N] or packed int32 words (pack_eligible)")
        if N == 0:
            raise ValueError("eligible is empty")
    dev = a_s.device
    out_s = torch.empty(U, topk, dtype=torch.float32, device=dev)
    out_i = torch.empty(U, topk, dtype=torch.int32, device=dev)
    if triple:
        out_g = torch.empty(U, topk, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().miner_topk_merge_grouped(_stream(dev), _ptr(a_s) if ka else None, _ptr(a_i) if ka else None, ka,
                                                     _ptr(b_s) if kb else None, _ptr(b_i) if kb else None, kb, U, topk,
                                                     _ptr(ok), N, _ptr(out_s), _ptr(out_i), _ptr(a_g) if ka else None,
                                                     _ptr(b_g) if kb else None, _ptr(out_g), interest_cap or 0)
        _lib.check(rc, "miner_topk_merge_grouped")
        return out_s, out_i, out_g
    with torch.cuda.device(dev):
        rc = _lib.lib().miner_topk_merge_capped(_stream(dev), _ptr(a_s) if ka else None, _ptr(a_i) if ka else None, ka,
                                                _ptr(b_s) if kb else None, _ptr(b_i) if kb else None, kb, U, topk,
                                                _ptr(ok), N, _ptr(out_s), _ptr(out_i),
                                                None if caps is None else _ptr(caps.cluster),
                                                0 if caps is None else caps.cluster.shape[0], 0 if caps is None else caps.cap)
    _lib.check(rc, "miner_topk_merge")
    return out_s, out_i


def update_topk(lists, user_mui: Tensor, user_proj: Optional[Tensor], news: Tensor, news_ids, *,
                score_type: str = "weighted", exclude_ids: Optional[Tensor] = None,
                eligible: Optional[Tensor] = None, news_bias=None, user_group: Optional[Tensor] = None,
                news_cluster=None, cluster_cap: Optional[int] = None, interest_cap: Optional[int] = None):
    """Incremental ranking: ``lists`` = (scores [U,k], ids [U,k]) ranked earlier for these users; the
    table rows ``news_ids`` (new or changed news) are ranked with rank_topk(news_ids=...) and merged
    in with merge_topk — a re-ranked news takes its fresh score. ``exclude_ids`` filters the fresh
    rows as in rank_topk; ``eligible`` filters them and also prunes expired news from ``lists``.
    Returns the new (scores [U,k], ids [U,k]); the cost follows len(news_ids), not the table.
    ``news_bias`` / ``user_group`` as in rank_topk: the fresh rows are ranked under the prior that
    ``lists`` was ranked under (a list ranked under another prior holds stale scores: rescore_topk).
    ``news_cluster`` / ``cluster_cap`` as in rank_topk: the fresh rows are ranked under the caps and
    merged with the capped merge. Exact: where the fresh ids are new to ``lists`` (disjoint id sets)
    and ``lists`` is the capped ranking of the old ids under the same table, the result is the
    capped ranking of the union, bit for bit. Stale, as a list under another prior is: a capped
    list holds only what its caps let through, so when ``eligible`` prunes an entry, or a re-ranked
    news comes back with a lower score, the same-cluster news that entry once displaced is no longer
    in the list and does not return — the result is within its caps, but may miss that news until
    the users are ranked again.
    ``lists`` may be a (scores, ids, interests) triple (rank_topk's ``return_interest``): the fresh
    rows are ranked with their interests and the result is a triple. ``interest_cap`` (triples only;
    not with news_cluster / cluster_cap) as in rank_topk: the fresh rows are ranked under the
    per-interest cap and merged with the grouped merge. Exact and stale exactly as under the
    per-cluster caps: where the fresh ids are new to ``lists`` and ``lists`` is the interest-capped
    ranking of the old ids for the same user vectors, the result is the interest-capped ranking of
    the union, bit for bit; but a capped list holds only what its caps let through, so when
    ``eligible`` prunes an entry, or a re-ranked news comes back with a lower score, the
    same-interest news that entry once displaced is no longer in the list and does not return —
    within its caps, but possibly missing that news until the users are ranked again. (And the
    interests in ``lists`` are those of the user vectors it was ranked with.) ``resume=`` is not
    offered: ``lists`` is a first page (a capped list from the top), not a later page of a walk."""
    triple = _is_triple(lists)
    if interest_cap is not None and not triple:
        raise ValueError("interest_cap needs lists with interests: a (scores, ids, interests) triple")
    if triple and (news_cluster is not None or cluster_cap is not None):
        raise ValueError("lists with interests cannot be updated under news_cluster / cluster_cap")
    old = _list_triple(lists, "lists") if triple else _list_pair(lists, "lists")
    k = old[0].shape[1]
    if k < 1:
        raise ValueError("lists must hold at least one entry per user")
    req = _request(user_mui.shape[0], news.shape[0], score_type=score_type, exclude_ids=exclude_ids, eligible=eligible,
                   news_ids=news_ids, news_bias=news_bias, user_group=user_group, news_cluster=news_cluster,
                   cluster_cap=cluster_cap, interest_cap=interest_cap, return_interest=triple)
    _, _, mui, proj, tab = _rank_operands(user_mui, user_proj, news, score_type)
    fresh = _rank(mui, proj, tab, k, req)
    return merge_topk(old, fresh, k, eligible=req.ok, news_cluster=None if req.caps is None else req.caps.cluster,
                      cluster_cap=cluster_cap, interest_cap=interest_cap)


def cap_topk(lists, news_cluster, cluster_cap: int, topk: Optional[int] = None):
    """The post-hoc cap of served lists (scores [U,k], ids [U,k]; k <= 256, rows in any order): the
    capped walk of each row (rank_topk's ``news_cluster`` / ``cluster_cap``), the best ``topk``
    (default k) kept entries, then (-inf, -1) — the capped merge with an empty first list. The cap of
    a list is prefix-exact: capping an uncapped top-k gives the first entries of the true capped
    list, so the result IS rank_topk's capped list wherever it fills ``topk`` or the input list was
    not full (then the input held every admissible news); a row that comes back short from a full
    input needs the capped ranker. Every group counts from 0: there is no ``resume=`` here."""
    caps = _caps(news_cluster, cluster_cap, None)
    _require_device(news_cluster)
    s, i = _list_pair(lists, "lists")
    if s.shape[1] < 1:
        raise ValueError("lists must hold at least one entry per user")
    return merge_topk((s[:, :0], i[:, :0]), (s, i), s.shape[1] if topk is None else topk, news_cluster=caps.cluster,
                      cluster_cap=caps.cap)


MAX_POOL = 256
_RELEVANCE = {"score": 0, "minmax": 1}          # MINER_DIVERSIFY_REL_* of include/miner_diversify.h


def _mmr_args(lam, relevance) -> tuple:
    """The checked (lambda, relevance code) of the diversity re-ranking."""
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0.0 <= lam <= 1.0:    # (NaN fails both)
        raise ValueError("lam must be a number in [0, 1]")
    if not isinstance(relevance, str) or relevance not in _RELEVANCE:
        raise ValueError(f"relevance must be one of {sorted(_RELEVANCE)}")
    return float(lam), _RELEVANCE[relevance]


def diversify_topk(lists, news: Tensor, topk: Optional[int] = None, *, lam: float = 0.7, relevance: str = "minmax",
                   return_positions: bool = False, return_objective: bool = False):
    """Diversity re-ranking (maximal marginal relevance) of per-user pools on the device: ``lists`` =
    (scores [U,P] fp32, ids [U,P] integer), P <= 256 — a list of rank_topk / merge_topk /
    rank_topk_deep[:, :256], or any rows of pairs, in the order given — re-ordered by a greedy walk
    that trades an entry's relevance against its cosine similarity, in the space of the table
    ``news`` [N, d] (fp16, bf16 or fp32; d as the ranker takes it), to what the walk already listed:

        pick the unlisted candidate p that maximises  lam · rel_p − (1 − lam) · max_{q listed} sim_pq

    ``topk`` times (default P), ties to the lower position. An entry is a candidate iff its id is in
    [0, N) and its score finite: the (-inf, -1) tail of a short list, ids outside the table and NaN /
    infinite scores are never listed and no row is read for them; a repeated id is a candidate at
    each position. ``relevance`` 'minmax' (default) scales the user's candidate scores to [0, 1]
    (rel = 0 when they are all equal) so that ``lam`` means the same for every user, 'score' takes
    them as they are. sim is the cosine of the table rows, the products accumulated in fp32 on the
    matrix cores, 0 for an all-zero row or a row that holds an inf / NaN. All arithmetic of the
    objective is fp32 (include/miner_diversify.h is the contract; tests/diversify_ref.py restates it).

    Returns (scores [U,topk] fp32, ids [U,topk] int32): the listed entries with their input scores
    bit for bit, then (-inf, -1) once the candidates ran out. A (scores, ids, interests) triple comes
    back as a triple, each entry with its interest (-1 in the tail). ``return_positions`` appends
    positions int32 [U,topk], where in the pool each entry stood (-1 in the tail);
    ``return_objective`` appends the fp32 objective each entry had when it was picked (-inf in the
    tail). lam = 1 lists the candidates by relevance, ties by position: a ranked list's own prefix.
    The result is a subset of the pool, so a pool ranked under caps (news_cluster / cluster_cap,
    interest_cap) keeps them; it is NOT in score order: not an input for merge_topk / update_topk /
    page_cursor. Users are independent: a batch gives what its users give alone, bit for bit. One
    launch, one workgroup per user; the price against the rank step: profiles/rk_diversify_ab.txt."""
    lam, rel = _mmr_args(lam, relevance)
    triple = _is_triple(lists)
    s, i, *g = _list_triple(lists, "lists") if triple else _list_pair(lists, "lists")
    U, P = s.shape
    if P < 1:
        raise ValueError("lists must hold at least one entry per user")
    topk = P if topk is None else topk
    if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= P:
        raise ValueError(f"topk must be an int in [1, {P}], the pool's width")
    if not isinstance(news, Tensor) or news.dim() != 2 or news.shape[0] < 1:
        raise ValueError("news must be a table [N, d] with N >= 1")
    dt = _code(news.dtype)
    N, d = news.shape
    if d < 1 or d > 1024 or d % (32 if dt == _lib.DTYPE_F32 else 64):
        raise ValueError(f"d = {d}: the table's width must be a multiple of 64 (float32: of 32), at most 1024")
    _require_device(s, i, *g, news)
    tab = news.contiguous()
    dev = tab.device
    if s.device != dev or i.device != dev or any(x.device != dev for x in g):
        raise ValueError("lists and news must be on one device")
    out_s = torch.empty(U, topk, dtype=torch.float32, device=dev)
    out_i = torch.empty(U, topk, dtype=torch.int32, device=dev)
    out_p = torch.empty(U, topk, dtype=torch.int32, device=dev)
    out_o = torch.empty(U, topk, dtype=torch.float32, device=dev) if return_objective else None
    with torch.cuda.device(dev):
        rc = _lib.lib().miner_topk_diversify(_stream(dev), dt, _ptr(tab), N, d, _ptr(s), _ptr(i), U, P, topk, lam, rel,
                                             _ptr(out_s), _ptr(out_i), _ptr(out_p), _ptr(out_o))
    _lib.check(rc, "miner_topk_diversify")
    out = (out_s, out_i)
    if triple:
        listed = out_p >= 0
        out += (torch.where(listed, g[0].gather(1, out_p.clamp(min=0).to(torch.int64)), -1).to(torch.int32),)
    if return_positions:
        out += (out_p,)
    if return_objective:
        out += (out_o,)
    return out


def rank_topk_diverse(user_mui: Tensor, user_proj: Optional[Tensor], news: Tensor, topk: int, *,
                      pool: Optional[int] = None, lam: float = 0.7, relevance: str = "minmax", **rank_kwargs):
    """rank_topk, then diversify_topk: the ``pool`` best news per user (default min(256, 4 · topk);
    topk <= pool <= 256) ranked with rank_topk(..., topk=pool, **rank_kwargs), re-ranked to ``topk`` by
    diversify_topk(..., lam=, relevance=) against the same table — bit for bit those two calls.
    Everything else is rank_topk's and passes through unchanged: score_type, exclude_ids, eligible,
    news_ids, news_bias / user_group, news_cluster / cluster_cap, interest_cap, after,
    return_interest (the result is then a triple). The page is a subset of the pool, so a pool ranked
    under caps keeps its caps. ``resume=`` is refused: a diversified page is not a page of a walk (it
    is not in score order and does not end where the next page would begin)."""
    if rank_kwargs.get("resume") is not None:
        raise ValueError("rank_topk_diverse: a diversified page is not a walk page, there is no resume=")
    lam, _ = _mmr_args(lam, relevance)
    if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= MAX_POOL:
        raise ValueError(f"topk must be an int in [1, {MAX_POOL}]")
    pool = min(MAX_POOL, 4 * topk) if pool is None else pool
    if isinstance(pool, bool) or not isinstance(pool, int) or not topk <= pool <= MAX_POOL:
        raise ValueError(f"pool must be an int in [topk, {MAX_POOL}]: the re-ranking chooses topk = {topk} of the pool")
    return diversify_topk(rank_topk(user_mui, user_proj, news, pool, **rank_kwargs), news, topk, lam=lam,
                          relevance=relevance)


MAX_TARGETS = 64


def _rank_operands(user_mui: Tensor, user_proj: Optional[Tensor], news: Tensor, score_type: str):
    """The checks and conversions rank_topk makes of the user vectors and the table."""
    st = _lib.SCORE_TYPES.get(score_type)
    if st is None or st == _lib.SCORE_NONE:
        raise ValueError("Invalid method of aggregating matching score")  # model.py:136
    _require_device(user_mui, user_proj, news)
    dtype = user_mui.dtype
    dt = _code(dtype)
    mui = _contig(user_mui, dtype)
    proj = _contig(user_proj, dtype) if st == _lib.SCORE_WEIGHTED else None
    if st == _lib.SCORE_WEIGHTED and proj is None:
        raise ValueError("score_type 'weighted' needs user_proj")
    tab = _contig(news, dtype)
    if mui.dim() != 3 or tab.dim() != 2 or tab.shape[1] != mui.shape[2] or (proj is not None and proj.shape != mui.shape):
        raise ValueError("shape mismatch between user vectors and the news table")
    return st, dt, mui, proj, tab


def _check_ids(ids, U: int, what: str) -> None:
    """Shape and dtype of an id matrix (before anything touches the device)."""
    if not _is_int(ids, 2) or ids.shape[0] != U:
        raise ValueError(f"{what} must be an integer [{U}, C] tensor")


def _id_matrix(ids: Tensor, U: int, N: int, what: str) -> Tensor:
    """An integer [U, C] tensor of news ids -> int64, ids outside [0, N) replaced by -1."""
    _check_ids(ids, U, what)
    _require_device(ids)
    ids = ids.to(torch.int64)
    return torch.where((ids >= 0) & (ids < N), ids, -1)


def _bits_at(words: Tensor, ids: Tensor) -> Tensor:
    """Eligibility of the news ``ids`` (int64, any shape, -1 = none) under the packed bitmap."""
    safe = ids.clamp(min=0)
    return (((words[safe >> 5].to(torch.int64) >> (safe & 31)) & 1) != 0) & (ids >= 0)


def _score_pairs(st, dt, mui, proj, tab, ids64: Tensor, pri: Optional[_Prior] = None, interest: bool = False):
    """scores [U, C]; with ``interest`` (scores, interests int32 [U, C]) from the one launch."""
    U, K, d = mui.shape
    C = ids64.shape[1]
    out = torch.empty(U, C, dtype=torch.float32, device=mui.device)
    intr = torch.empty(U, C, dtype=torch.int32, device=mui.device) if interest else None
    if U == 0 or C == 0:
        return (out, intr) if interest else out
    ids = ids64.to(torch.int32).contiguous()
    with torch.cuda.device(mui.device):
        rc = _lib.lib().miner_score_pairs_interest(_stream(mui.device), dt, st, _ptr(mui), _ptr(proj), _ptr(tab), U,
                                                   tab.shape[0], d, K, _ptr(ids), C, _ptr(out), *_prior_args(pri),
                                                   _ptr(intr))
    _lib.check(rc, "miner_score_pairs")
    return (out, intr) if interest else out


def score_pairs(user_mui: Tensor, user_proj: Optional[Tensor], news: Tensor, cand_ids: Tensor, *,
                score_type: str = "weighted", news_bias=None, user_group: Optional[Tensor] = None,
                return_interest: bool = False):
    """The click score of chosen pairs: scores[u, c] of (user u, news[cand_ids[u, c]]), fp32 [U, C] —
    bit for bit what rank_topk computes for that pair, from the cached user vectors. cand_ids [U, C]
    of any integer dtype, any order, repeats allowed; an id outside [0, N) (a -1 padding) gives -inf.
    Only the U x C rows are read: the second stage of a recommender, or the refresh of a served list
    (rescore_topk). ``news_bias`` / ``user_group`` as in rank_topk: the prior of the pair's news is
    added (an id outside [0, N) stays -inf). ``return_interest``: (scores, interests) — interests
    int32 [U, C], the dominant interest of each pair (rank_topk's ``return_interest``: the lowest k
    whose logit, or M_k under 'max', equals the maximum the score's reduction over K found; -1 for
    an id outside [0, N); ValueError under 'mean'), from the same launch: the scores keep their bits
    and the prior does not enter the interest."""
    if return_interest:
        _dominant_interest(score_type)
    _check_ids(cand_ids, user_mui.shape[0], "cand_ids")
    pri = _prior(news_bias, user_group, user_mui.shape[0], news.shape[0])
    _require_device(news_bias, user_group)
    st, dt, mui, proj, tab = _rank_operands(user_mui, user_proj, news, score_type)
    return _score_pairs(st, dt, mui, proj, tab, _id_matrix(cand_ids, mui.shape[0], tab.shape[0], "cand_ids"), pri,
                        return_interest)


def _better(s: Tensor, i: Tensor, s2: Tensor, i2: Tensor) -> Tensor:
    """The ranker's total order: (s, i) before (s2, i2)."""
    return (s > s2) | ((s == s2) & (i < i2))


def _rank_of(user_mui, user_proj, news, target_ids, score_type, exclude_ids, eligible, pri: Optional[_Prior] = None):
    """rank_of under a checked prior, plus the number of news in each user's list (int64 [U])."""
    _check_ids(target_ids, user_mui.shape[0], "target_ids")
    if not 1 <= target_ids.shape[1] <= MAX_TARGETS:
        raise ValueError(f"target_ids holds {target_ids.shape[1]} targets per user, outside [1, {MAX_TARGETS}]")
    if exclude_ids is not None:
        _check_ids(exclude_ids, user_mui.shape[0], "exclude_ids")
        if exclude_ids.shape[1] > MAX_L:
            raise ValueError(f"exclude_ids holds {exclude_ids.shape[1]} ids per user, more than {MAX_L}")
    st, dt, mui, proj, tab = _rank_operands(user_mui, user_proj, news, score_type)
    U, K, d = mui.shape
    N = tab.shape[0]
    dev = mui.device
    tid = _id_matrix(target_ids, U, N, "target_ids")
    T = tid.shape[1]
    _require_device(exclude_ids, eligible)
    ex = None
    if exclude_ids is not None:
        ex = _id_matrix(exclude_ids, U, N, "exclude_ids")
        if ex.shape[1] == 0:
            ex = None
    ok = None if eligible is None else _eligible_words(eligible, N)
    tgt_s = _score_pairs(st, dt, mui, proj, tab, tid, pri)      # with a prior: biased, as the stream's scores are
    counts = torch.empty(U, T, dtype=torch.int32, device=dev)
    if U:
        tid32 = tid.to(torch.int32).contiguous()
        with torch.cuda.device(dev):
            rc = _lib.lib().miner_rank_count_biased(_stream(dev), dt, st, _ptr(mui), _ptr(proj), _ptr(tab), U, N, d, K,
                                                    _ptr(tgt_s), _ptr(tid32), T, _ptr(ok), _ptr(counts), *_prior_args(pri))
        _lib.check(rc, "miner_rank_count")
    appears = (tid >= 0) & ~torch.isnan(tgt_s)
    if ok is not None:
        appears &= _bits_at(ok, tid)
    n_ok = N if ok is None else int(_bits_at(ok, torch.arange(N, device=dev)).sum())
    survivors = torch.full((U,), n_ok, dtype=torch.int64, device=dev)
    ranks = counts.to(torch.int64)
    if ex is not None and U:
        # the excluded news the kernel counted: distinct, in range, eligible, ranking before the target
        # — their scores are the stream's own bits (score_pairs), so the correction is exact
        ex = torch.sort(ex, dim=1).values
        ex[:, 1:] = torch.where(ex[:, 1:] == ex[:, :-1], -1, ex[:, 1:])
        ex_s = _score_pairs(st, dt, mui, proj, tab, ex, pri)
        live = ex >= 0 if ok is None else _bits_at(ok, ex)
        survivors -= live.sum(dim=1)
        E = ex.shape[1]
        step = max(1, (1 << 26) // max(1, E * T))             # users per [u, E, T] comparison block
        for u0 in range(0, U, step):
            sl = slice(u0, u0 + step)
            before = live[sl, :, None] & _better(ex_s[sl, :, None], ex[sl, :, None], tgt_s[sl, None, :], tid[sl, None, :])
            ranks[sl] -= before.sum(dim=1)
            appears[sl] &= ~(ex[sl, :, None] == tid[sl, None, :]).any(dim=1)
    ranks = torch.where(appears, ranks, -1).to(torch.int32)
    return ranks, tgt_s, survivors


def rank_of(user_mui: Tensor, user_proj: Optional[Tensor], news: Tensor, target_ids: Tensor, *,
            score_type: str = "weighted", exclude_ids: Optional[Tensor] = None, eligible: Optional[Tensor] = None,
            news_bias=None, user_group: Optional[Tensor] = None):
    """Exact full-corpus ranks: (ranks int32 [U, T], scores fp32 [U, T]) for target_ids [U, T]
    (integer, T <= 64). ranks[u, j] is the 0-based position news target_ids[u, j] holds in user u's
    complete filtered list — what rank_topk with the same ``exclude_ids`` / ``eligible`` would return
    if topk were N — and -1 if it would not appear (id outside [0, N), not eligible, in
    exclude_ids[u], or a NaN score). The table is streamed once for all T targets and no list is
    kept (miner_rank_count); the targets' scores come from score_pairs, whose bits are the stream's
    own, so the count is exact and a tie ranks by id. The exclusion list is a correction on the device:
    its distinct, in-range, eligible ids that rank before the target are subtracted. ``news_bias`` /
    ``user_group`` as in rank_topk: targets, stream and correction all use the biased score, so the
    rank is exact under the prior too (a target whose biased score is NaN gets -1)."""
    pri = _prior(news_bias, user_group, user_mui.shape[0], news.shape[0])
    _require_device(news_bias, user_group)
    return _rank_of(user_mui, user_proj, news, target_ids, score_type, exclude_ids, eligible, pri)[:2]


def corpus_metrics(ranks: Tensor, n_ranked: Optional[Tensor] = None, *, ks=(5, 10)):
    """Full-ranking metrics of ranks [U, T] (0-based rank of each held-out click in the user's list
    over the corpus; -1: no target in that slot). Pure torch, any device. Returns (per_user, means):
    per_user[name] a float64 [U] tensor (NaN for a user with no target), means[name] its mean over
    the users that have at least one target.
      recall@k  share of the user's targets ranked below k;  hit@k  1 if any is
      mrr       mean over the targets of 1 / (rank + 1)  (the reference's compute_mrr_score)
      ndcg@k    binary gains, discount log2(rank + 2), ideal DCG over min(#targets, k) positions
      auc       (with n_ranked [U], the number of news in each user's list) the share of (target,
                non-target) pairs the strict total order puts the right way round; NaN where every
                ranked news is a target."""
    if ranks.dim() != 2 or ranks.is_floating_point():
        raise ValueError("ranks must be an integer [U, T] tensor")
    r = ranks.to(torch.int64)
    has = r >= 0
    m = has.sum(dim=1).to(torch.float64)
    some = m > 0
    nan = torch.full_like(m, float("nan"))
    rf = r.clamp(min=0).to(torch.float64)
    per = {}
    for k in ks:
        below = has & (r < k)
        per[f"recall@{k}"] = torch.where(some, below.sum(dim=1) / m, nan)
        per[f"hit@{k}"] = torch.where(some, below.any(dim=1).to(torch.float64), nan)
        dcg = torch.where(below, 1.0 / torch.log2(rf + 2.0), 0.0).sum(dim=1)
        pos = torch.arange(min(k, r.shape[1]), device=r.device, dtype=torch.float64)
        ideal = torch.where(pos[None, :] < m[:, None], 1.0 / torch.log2(pos + 2.0)[None, :], 0.0).sum(dim=1)
        per[f"ndcg@{k}"] = torch.where(some, dcg / ideal, nan)
    per["mrr"] = torch.where(some, torch.where(has, 1.0 / (rf + 1.0), 0.0).sum(dim=1) / m, nan)
    if n_ranked is not None:
        n = n_ranked.to(r.device, torch.float64)
        # target i (in rank order) has n - 1 - rank_i news behind it, m - 1 - i of them targets
        good = torch.where(has, n[:, None] - 1.0 - rf, 0.0).sum(dim=1) - m * (m - 1.0) / 2.0
        per["auc"] = torch.where(some & (n > m), good / (m * (n - m)), nan)
    means = {}
    for name, v in per.items():
        v = v[some & ~torch.isnan(v)]
        means[name] = float(v.mean()) if v.numel() else float("nan")
    return per, means


def rescore_topk(lists, user_mui: Tensor, user_proj: Optional[Tensor], news: Tensor, *,
                 score_type: str = "weighted", eligible: Optional[Tensor] = None, news_bias=None,
                 user_group: Optional[Tensor] = None):
    """Served lists (scores [U,k], ids [U,k]) after the users' vectors changed: the lists' ids are
    scored again with score_pairs and re-sorted (and, with ``eligible``, pruned) by merge_topk. Returns
    lists of the same width — for each user, rank_topk(news_ids=<its old ids>) bit for bit, under the
    prior ``news_bias`` / ``user_group`` if one is given (also the way to move a list to a new prior)."""
    pri = _prior(news_bias, user_group, user_mui.shape[0], news.shape[0])
    _, ids = _list_pair(lists, "lists")
    if ids.shape[1] < 1:
        raise ValueError("lists must hold at least one entry per user")
    _require_device(news_bias, user_group)
    st, dt, mui, proj, tab = _rank_operands(user_mui, user_proj, news, score_type)
    fresh = _score_pairs(st, dt, mui, proj, tab, _id_matrix(ids, mui.shape[0], tab.shape[0], "lists"), pri)
    empty = (fresh[:, :0], ids[:, :0])
    return merge_topk(empty, (fresh, ids), ids.shape[1], eligible=eligible)


def _exclusions(exclude_ids: Optional[Tensor], exclude_history: bool, his_ids: Tensor, his_mask: Tensor):
    """The exclusion matrix of rank_corpus / evaluate_corpus: ``exclude_ids`` [U, E], behind each
    user's own history when ``exclude_history``; None when there is neither."""
    U = his_ids.shape[0]
    excl = exclude_ids
    if excl is not None and (excl.dim() != 2 or excl.shape[0] != U):
        raise ValueError(f"exclude_ids must be [{U}, E]")
    if exclude_history:
        seen = torch.where(his_mask.to(torch.bool), his_ids, -1).to(torch.int32)   # padded slots exclude nothing
        excl = seen if excl is None else torch.cat([seen, excl.to(torch.int32)], dim=1)
    if excl is not None and excl.shape[1] > MAX_L:
        raise ValueError(f"{excl.shape[1]} excluded ids per user, more than {MAX_L}")
    return excl


def evaluate_corpus(news: Tensor, his_ids: Tensor, his_mask: Tensor, packed: EncoderWeights, target_ids: Tensor, *,
                    ks=(5, 10), batch: int = 16384, exclude_history: bool = True,
                    exclude_ids: Optional[Tensor] = None, eligible: Optional[Tensor] = None,
                    his_bias: Optional[Tensor] = None, score_type: str = "weighted", news_bias=None,
                    user_group: Optional[Tensor] = None):
    """The full-ranking evaluation protocol on one GPU's share of the users: rank_corpus's loop with
    rank_of in place of rank_topk. Every user is encoded from its history and each held-out click
    target_ids[u, j] (-1: no target in that slot) is ranked among all N news, the user's history
    (``exclude_history``) and ``exclude_ids`` left out, ``eligible`` as in rank_topk. Returns
    (ranks int32 [U, T], metrics): corpus_metrics' means — recall@k, hit@k, ndcg@k, mrr, auc. Each
    user's ranks are independent of the batching. ``news_bias`` / ``user_group`` [U] as in rank_topk
    (checked once, sliced per batch): the ranks under the prior."""
    if batch <= 0:
        raise ValueError("batch must be positive")
    U = his_ids.shape[0]
    dev = news.device
    # the prior checked and the bitmap packed once (rank_of's exclusions are an id matrix of its own)
    req = _request(U, news.shape[0], score_type=score_type, eligible=eligible, news_bias=news_bias, user_group=user_group)
    _require_device(news, his_ids, his_mask, target_ids, exclude_ids)
    excl = _exclusions(exclude_ids, exclude_history, his_ids, his_mask)
    if target_ids.dim() != 2 or target_ids.shape[0] != U:
        raise ValueError(f"target_ids must be [{U}, T]")
    ranks = torch.empty(U, target_ids.shape[1], dtype=torch.int32, device=dev)
    survivors = torch.empty(U, dtype=torch.int64, device=dev)
    with_proj = score_type == "weighted"
    for u0 in range(0, U, batch):
        u1 = min(U, u0 + batch)
        mui, proj = encode_users(news, his_mask[u0:u1], packed, his_ids=his_ids[u0:u1],
                                 his_bias=None if his_bias is None else his_bias[u0:u1], with_proj=with_proj)
        ranks[u0:u1], _, survivors[u0:u1] = _rank_of(mui, proj, news, target_ids[u0:u1], score_type,
                                                     None if excl is None else excl[u0:u1], req.ok,
                                                     None if req.prior is None else req.prior.users(u0, u1))
    return ranks, corpus_metrics(ranks, survivors, ks=ks)[1]


def rank_corpus(news: Tensor, his_ids: Tensor, his_mask: Tensor, packed: EncoderWeights, topk: int, *,
                his_bias: Optional[Tensor] = None, score_type: str = "weighted", batch: int = 16384,
                out: Optional[tuple] = None, exclude_history: bool = False, exclude_ids: Optional[Tensor] = None,
                eligible: Optional[Tensor] = None, news_ids=None, news_bias=None,
                user_group: Optional[Tensor] = None, news_cluster=None, cluster_cap: Optional[int] = None,
                after=None, interest_cap: Optional[int] = None, return_interest: bool = False, resume=None):
    """BASELINE config 5 on one GPU's share of the users: every user (his_ids [U,L] into the news
    table [N,d], his_mask [U,L]) encoded and ranked against the whole table, ``batch`` users per
    encode + rank pair so that the [batch,K,d] user vectors are all that is ever held (125,000 users
    at K = 64, d = 768, fp16 would be 24.6 GB of mui + proj at once). Returns (scores [U,topk] fp32,
    ids [U,topk] int32), best first: each user's list is independent of the batching
    (tests/test_gpu_fullsize.py). ``out`` = preallocated (scores, ids) to write into.

    ``exclude_history`` keeps each user's own clicked news (the unmasked his_ids) out of its list,
    ``exclude_ids`` [U,E] further ids, together at most 256 per user; ``eligible`` and ``news_ids`` (rank only these table rows) as in
    rank_topk; ``news_bias`` / ``user_group`` [U] (a score prior, checked once and sliced per batch) too;
    ``news_cluster`` / ``cluster_cap`` (per-cluster caps, checked and converted once) too; ``after``
    (keyset cursors [U], checked once and sliced per batch; never together with the caps) too;
    ``interest_cap`` / ``return_interest`` (per-interest caps and the listed pairs' dominant interests,
    as in rank_topk) too: with ``return_interest`` the result, and ``out``, is a (scores, ids,
    interests [U,topk] int32) triple. ``resume`` (a WalkState for all U users, checked once and sliced
    per batch: the capped walk continued, as in rank_topk — it needs a cap and excludes ``after``) too."""
    if batch <= 0:
        raise ValueError("batch must be positive")
    U = his_ids.shape[0]
    dev = news.device
    if out is not None and len(out) != (3 if return_interest else 2):
        raise ValueError("out must be (scores, ids), or (scores, ids, interests) with return_interest")
    # (the exclusion matrix is put together before the options are checked: the request checks it too)
    excl = _exclusions(exclude_ids, exclude_history, his_ids, his_mask)
    # checked, packed and canonicalised once; sliced per batch
    req = _request(U, news.shape[0], score_type=score_type, exclude_ids=excl, eligible=eligible, news_ids=news_ids,
                   news_bias=news_bias, user_group=user_group, news_cluster=news_cluster, cluster_cap=cluster_cap,
                   after=after, interest_cap=interest_cap, return_interest=return_interest, resume=resume)
    _require_device(news, his_ids, his_mask)
    res = tuple(out) if out is not None else (torch.empty(U, topk, dtype=torch.float32, device=dev),
                                              torch.empty(U, topk, dtype=torch.int32, device=dev)) + \
        ((torch.empty(U, topk, dtype=torch.int32, device=dev),) if return_interest else ())
    with_proj = score_type == "weighted"
    for u0 in range(0, U, batch):
        u1 = min(U, u0 + batch)
        mui, proj = encode_users(news, his_mask[u0:u1], packed, his_ids=his_ids[u0:u1],
                                 his_bias=None if his_bias is None else his_bias[u0:u1], with_proj=with_proj)
        _, _, mui, proj, tab = _rank_operands(mui, proj, news, score_type)
        for dst, src in zip(res, _rank(mui, proj, tab, topk, req.users(u0, u1))):
            dst[u0:u1] = src
    return res
