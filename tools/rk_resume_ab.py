"""Config-5 ranker step (2,048 users x 200,000 news, L = 200, K = 64, d = 768, fp16, weighted, top-100)
in one process, interleaved on the same inputs:
  (a) a library built from the parent commit (loaded by path) and this build: the unfiltered, filtered
      (a bitmap with every bit set), 5 % subset, biased (G = 1), capped (20,000 stories of 10 news,
      cap 1), cursor (the second page) and interest (cap 10) steps — this build's lists must equal the
      parent's bit for bit and its median must lie within the spread (max - min) of the parent's own
      repeats (each parent / this-build pair swaps places every repeat),
  (b) this build's resumed step (miner_rank_topk_resume) with the empty state against the parent's
      capped step,
  (c) page 2 and page 5 of the stories at cap 1 and of 300 publishers at cap 3 (states chained with
      miner_walk_advance), against the parent's capped step and cursor step,
      and the same two cursors with the tables emptied (the time only: what the table itself costs),
  (d) the same for interest_cap = 10,
  (e) corpus.rank_topk_deep_capped at topk = 1,000 (the stories, cap 1) against four resumed pages
      and against rank_topk_deep (the uncapped deep list: the cursor form, unchanged since the parent),
  (f) miner_walk_advance for 2,048 x (1,024 + 100): a full table of 1,024 groups and a page of 100,
  (g) the two libraries' sizes.
Every resumed list is checked: pages 1 .. 5 are disjoint, no group above its cap over the
concatenation, and the concatenation's first 256 entries equal the capped (or interest-capped)
top-256 call without a state, bit for bit. The parent library is recognised by having no
miner_rank_topk_resume symbol (the ABI number is the same). The exit status is 0 only if every list
of (a) is identical, every median of (a) lies inside the parent's spread and every check of the new
forms holds.
    python tools/rk_resume_ab.py PARENT_LIB [reps] [out.txt] [U] [N]"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from miner_amd import _lib, corpus, synthetic  # noqa: E402

dev = "cuda:0"
parent_path = sys.argv[1]
R = int(sys.argv[2]) if len(sys.argv) > 2 else 7
out_path = sys.argv[3] if len(sys.argv) > 3 else None
U = int(sys.argv[4]) if len(sys.argv) > 4 else 2048
N = int(sys.argv[5]) if len(sys.argv) > 5 else 200000
L, K, d, Dc, topk = 200, 64, 768, 200, 100
dt = torch.float16
g = torch.Generator(device=dev).manual_seed(5)
table = (torch.randn((N, d), generator=g, device=dev) / d ** 0.5).to(dt)
hid = torch.randint(0, N, (U, L), generator=g, device=dev, dtype=torch.int32)
mask = torch.ones((U, L), dtype=torch.bool, device=dev)
W1, Q, W2 = synthetic.init_weights(5, d, Dc, K, device=dev)
pk = corpus.pack_encoder(W1, Q, W2, dtype=dt)
mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
okw = corpus.pack_eligible(torch.ones(N, dtype=torch.bool, device=dev))
stories = (torch.randperm(N, generator=g, device=dev) // 10).to(torch.int32).contiguous()
publishers = torch.randint(0, 300, (N,), generator=g, device=dev, dtype=torch.int32)
sub = torch.sort(torch.randperm(N, generator=g, device=dev)[:N // 20]).values.to(torch.int32).contiguous()   # 5 %
torch.cuda.synchronize()

parent = ctypes.CDLL(parent_path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # its own symbols, not this build's
for name in ("miner_rank_topk", "miner_rank_topk_filtered", "miner_rank_topk_subset", "miner_rank_topk_biased",
             "miner_rank_topk_capped", "miner_rank_topk_after", "miner_rank_topk_interest"):
    getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
parent.miner_abi_version.restype = ctypes.c_int
lib = _lib.lib()
assert parent.miner_abi_version() == _lib.ABI_VERSION and not hasattr(parent, "miner_rank_topk_resume"), \
    "PARENT_LIB is not the parent commit's library"
F16, W = _lib.DTYPE_F16, _lib.SCORE_WEIGHTED
stream = lambda: torch.cuda.current_stream().cuda_stream
ptr = lambda x: None if x is None else x.data_ptr()
head = lambda: (stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K)

s0 = torch.empty(U, topk, dtype=torch.float32, device=dev)
i0 = torch.empty(U, topk, dtype=torch.int32, device=dev)
assert lib.miner_rank_topk(*head(), topk, ptr(s0), ptr(i0)) == 0
bias = (float(s0.std()) * torch.randn((1, N), generator=g, device=dev)).contiguous()
cur_s, cur_i = corpus.page_cursor((s0, i0))            # the second page


def outs(k=topk):
    return torch.empty(U, k, dtype=torch.float32, device=dev), torch.empty(U, k, dtype=torch.int32, device=dev)


def call(fn, *args):
    s, i = outs()

    def run():
        rc = fn(s, i, *args)
        assert rc == 0, rc
        return s, i
    return run


def plain(h):
    return call(lambda s, i: h.miner_rank_topk(*head(), topk, ptr(s), ptr(i)))


def filtered(h):
    return call(lambda s, i: h.miner_rank_topk_filtered(*head(), topk, None, 0, ptr(okw), ptr(s), ptr(i), None, 0))


def subset(h):
    return call(lambda s, i: h.miner_rank_topk_subset(*head(), topk, None, 0, None, ptr(sub), sub.numel(), ptr(s), ptr(i), None, 0))


def biased(h):
    return call(lambda s, i: h.miner_rank_topk_biased(*head(), topk, None, 0, None, None, -1, ptr(s), ptr(i), None, 0,
                                                      ptr(bias), 1, None))


def capped(h):
    return call(lambda s, i: h.miner_rank_topk_capped(*head(), topk, None, 0, None, None, -1, ptr(s), ptr(i), None, 0, None, 0,
                                                      None, ptr(stories), 1))


def cursor(h):
    return call(lambda s, i: h.miner_rank_topk_after(*head(), topk, None, 0, None, None, -1, ptr(s), ptr(i), None, 0, None, 0,
                                                     None, None, 0, ptr(cur_s), ptr(cur_i)))


def interest(h):
    gi = torch.empty(U, topk, dtype=torch.int32, device=dev)
    return call(lambda s, i: h.miner_rank_topk_interest(*head(), topk, None, 0, None, None, -1, ptr(s), ptr(i), None, 0, None, 0,
                                                        None, None, 0, None, None, 10, ptr(gi)))


def resumed(state, clus, cap, icap):
    s, i = outs()
    gi = torch.empty(U, topk, dtype=torch.int32, device=dev) if icap else None

    def run():
        rc = lib.miner_rank_topk_resume(*head(), topk, None, 0, None, None, -1, ptr(s), ptr(i), None, 0, None, 0, None,
                                        ptr(clus), cap, ptr(state.scores), ptr(state.ids), icap, ptr(gi), ptr(state.groups),
                                        ptr(state.counts), ptr(state.n_used), state.capacity)
        assert rc == 0, rc
        return (s, i, gi) if icap else (s, i)
    return run


def walk_pages(clus, cap, icap, pages=5):
    """states[j]: the state before page j + 1; lists[j]: page j + 1 (through the Python entries)."""
    kw = dict(interest_cap=icap, return_interest=True) if icap else dict(news_cluster=clus, cluster_cap=cap)
    state, states, lists = corpus.start_walk(U, dev), [], []
    for _ in range(pages):
        states.append(state)
        page = corpus.rank_topk(mui, proj, table, topk, resume=state, **kw)
        lists.append(page)
        state = corpus.advance_walk(state, page, news_cluster=None if icap else clus)
    return states, lists


WALKS = {"stories_cap1": (stories, 1, 0), "publishers_cap3": (publishers, 3, 0), "interest_cap10": (None, 0, 10)}
walks = {n: walk_pages(*a) for n, a in WALKS.items()}

FORMS = (("plain", plain), ("filtered", filtered), ("subset5", subset), ("biased", biased), ("capped", capped),
         ("cursor", cursor), ("interest", interest))
PAIRS = [(f"a_parent_{n}", f"a_this_{n}") for n, _ in FORMS]
VARIANTS = {}
for n, f in FORMS:
    VARIANTS[f"a_parent_{n}"], VARIANTS[f"a_this_{n}"] = f(parent), f(lib)
VARIANTS["b_resume_empty_state"] = resumed(walks["stories_cap1"][0][0], stories, 1, 0)
for n, (clus, cap, icap) in WALKS.items():
    for page in (2, 5):
        VARIANTS[f"{'d' if icap else 'c'}_{n}_page{page}"] = resumed(walks[n][0][page - 1], clus, cap, icap)
# (the time only: the same cursors with the tables emptied — no lookup, no saturated groups; other lists)
for page in (2, 5):
    st_ = walks["stories_cap1"][0][page - 1]
    bare = corpus.WalkState(st_.scores, st_.ids, st_.groups, st_.counts, torch.zeros_like(st_.n_used), st_.overflow)
    VARIANTS[f"c_stories_cap1_page{page}_table_emptied"] = resumed(bare, stories, 1, 0)
deep_kw = dict(news_cluster=stories, cluster_cap=1)
VARIANTS["e_deep_capped_1000"] = lambda: corpus.rank_topk_deep_capped(mui, proj, table, 1000, **deep_kw)
VARIANTS["e_rank_topk_deep_1000"] = lambda: corpus.rank_topk_deep(mui, proj, table, 1000)
full = corpus.WalkState(cur_s, cur_i, (2 * torch.arange(1024, device=dev, dtype=torch.int32)).repeat(U, 1).contiguous(),
                        torch.ones(U, 1024, dtype=torch.int32, device=dev), torch.full((U,), 1024, dtype=torch.int32, device=dev),
                        torch.zeros(U, dtype=torch.uint8, device=dev))
half_new = (s0, i0, torch.randint(0, 2048, (U, topk), generator=g, device=dev, dtype=torch.int32))
VARIANTS["f_walk_advance_1024_plus_100"] = lambda: (corpus.advance_walk(full, half_new).n_used,)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


ms, res = {v: [] for v in VARIANTS}, {}
for v, fn in VARIANTS.items():                                     # warm-up, and the results to compare
    res[v] = tuple(x.clone() for x in fn())
torch.cuda.synchronize()
names = list(VARIANTS)
for rep in range(R):
    # each gate pair swaps places every repeat: the same code must not be told apart by what ran before it
    order = list(names)
    if rep % 2:
        for a_, b_ in PAIRS:
            ia, ib = order.index(a_), order.index(b_)
            order[ia], order[ib] = order[ib], order[ia]
    for v in order:
        ms[v].append(timed(VARIANTS[v]))

bits = lambda x: x.view(torch.int32)
same_lists = lambda a, b: all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def walk_ok(name):
    """pages 1 .. 5: disjoint ids, no group above its cap over the concatenation, the first 256 the
    capped top-256 without a state; the timed pages equal the Python entries' pages"""
    clus, cap, icap = WALKS[name]
    lists = walks[name][1]
    ids = torch.cat([p[1] for p in lists], dim=1)
    srt = torch.sort(ids, dim=1).values
    disjoint = bool(((srt[:, 1:] != srt[:, :-1]) | (srt[:, 1:] < 0)).all())
    grp = torch.cat([p[2] for p in lists], dim=1) if icap else clus[ids.clamp(min=0).long()]
    c = torch.where((ids >= 0) & (grp >= 0), grp, -1 - torch.arange(ids.shape[1], device=dev, dtype=torch.int32)[None, :])
    cs = torch.sort(c, dim=1).values
    lim = icap or cap
    within = bool((cs[:, lim:] != cs[:, :-lim]).all())
    kw = dict(interest_cap=icap) if icap else dict(news_cluster=clus, cluster_cap=cap)
    top = corpus.rank_topk(mui, proj, table, 256, **kw)
    prefix = torch.equal(ids[:, :256], top[1]) and torch.equal(bits(torch.cat([p[0] for p in lists], dim=1)[:, :256]), bits(top[0]))
    timed_same = all(same_lists(res[f"{'d' if icap else 'c'}_{name}_page{pg}"], lists[pg - 1]) for pg in (2, 5))
    return disjoint and within and prefix and timed_same


checks = {n: walk_ok(n) for n in WALKS}
checks["b_resume_empty_state"] = same_lists(res["b_resume_empty_state"], res["a_parent_capped"])
four = torch.cat([p[1] for p in walks["stories_cap1"][1][:4]], dim=1)
checks["e_deep_capped_1000"] = torch.equal(res["e_deep_capped_1000"][1][:, :400], four)
med = {v: statistics.median(x) for v, x in ms.items()}
lines = [f"rk_resume_ab: U={U} N={N} L={L} K={K} d={d} fp16 weighted topk={topk}, {R} interleaved repeats, ms per call; "
         f"stories: {int(stories.max()) + 1} clusters of 10, cap 1; publishers: 300 clusters, cap 3; subset: {sub.numel()} ids"]
for v in VARIANTS:
    x = ms[v]
    lines.append(f"{v:34s} median {med[v]:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}  "
                 f"spread {max(x) - min(x):6.3f}  all {[round(t, 3) for t in x]}")
gates, inside = [], []
for a_, b_ in PAIRS:
    diff = med[b_] - med[a_]
    spread = max(ms[a_]) - min(ms[a_])
    same = same_lists(res[a_], res[b_])
    gates.append(same)
    inside.append(abs(diff) <= spread)
    lines.append(f"(a) this - parent {b_[7:]:9s}: {diff:+.3f} ms; the parent's own spread {spread:.3f} ms -> "
                 f"{'within' if abs(diff) <= spread else 'OUTSIDE'} it; lists identical: {same}")
pc, pcs, pcur, pflt = med["a_parent_capped"], max(ms["a_parent_capped"]) - min(ms["a_parent_capped"]), med["a_parent_cursor"], \
    med["a_parent_filtered"]
v = "b_resume_empty_state"
lines.append(f"(b) {v}: {med[v]:8.3f} ms = {med[v] / pc:.3f} x the parent's capped step ({pc:.3f}, spread {pcs:.3f}): "
             f"{'within' if abs(med[v] - pc) <= pcs else 'OUTSIDE'} its spread; lists identical to it: {checks[v]}")
incr = (pc - pflt) + (pcur - pflt)
for n, (clus, cap, icap) in WALKS.items():
    for page in (2, 5):
        v = f"{'d' if icap else 'c'}_{n}_page{page}"
        base_ = med["a_parent_interest"] if icap else pc
        lines.append(f"({'d' if icap else 'c'}) {v}: {med[v]:8.3f} ms = {med[v] / base_:.3f} x the parent's "
                     f"{'interest' if icap else 'capped'} step ({base_:.3f}) = {med[v] / pcur:.3f} x its cursor step ({pcur:.3f}); over "
                     f"the filtered step ({pflt:.3f}): {med[v] - pflt:+.3f} ms against the capped + cursor increments {incr:+.3f}"
                     f"{'' if page == 2 else f'; pages 1-5 disjoint, within the cap, first 256 == the call without a state: {checks[n]}'}")
for page in (2, 5):
    v, w = f"c_stories_cap1_page{page}_table_emptied", f"c_stories_cap1_page{page}"
    lines.append(f"(c) {v}: {med[v]:8.3f} ms (the same cursor, n_used = 0: the search skipped and no group used up; other lists): "
                 f"the table costs {med[w] - med[v]:+.3f} ms of page {page}'s {med[w]:.3f}")
pages4 = med["b_resume_empty_state"] + 3 * med["c_stories_cap1_page2"]
lines.append(f"(e) rank_topk_deep_capped topk=1000 (4 pages): {med['e_deep_capped_1000']:8.3f} ms = "
             f"{med['e_deep_capped_1000'] / pages4:.3f} x four resumed pages ({pages4:.3f}: page 1 + 3 x page 2) = "
             f"{med['e_deep_capped_1000'] / med['e_rank_topk_deep_1000']:.3f} x rank_topk_deep ({med['e_rank_topk_deep_1000']:.3f}); "
             f"its first 400 ids == pages 1-4 of 100: {checks['e_deep_capped_1000']}")
lines.append(f"(f) miner_walk_advance {U} x (1024 + {topk}), outputs allocated per call: {med['f_walk_advance_1024_plus_100']:8.4f} ms")
lines.append(f"(g) library size: parent {os.path.getsize(parent_path)} bytes, this build {os.path.getsize(_lib.LIB_PATH)} bytes")
text = "\n".join(lines)
print(text, flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
sys.exit(0 if all(gates) and all(inside) and all(checks.values()) else 1)
