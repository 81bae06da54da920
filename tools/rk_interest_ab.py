"""Config-5 ranker step (2,048 users x 200,000 news, L = 200, K = 64, d = 768, fp16, weighted, top-100)
in one process, interleaved on the same inputs:
  (a) a library built from the parent commit (loaded by path): its unfiltered, filtered (a bitmap
      with every bit set), 5 % subset, biased (G = 1), capped (20,000 stories of 10 news, cap 1) and
      cursor (the second page) steps,
  (b) this build, the same six calls — each one's lists must equal (a)'s bit for bit and its median
      must lie within the spread (max - min) of (a)'s own repeats: the instantiations that existed
      are unchanged (each (a)/(b) pair swaps places every repeat),
  (c) this build's interest-capped step (miner_rank_topk_interest) at cap 1, 3 and 10, with the
      interests returned, against this build's capped step (the stories at cap 1) and against the
      filtered step; the same under the prior, against the biased step,
  (d) the pair form with interests (miner_score_pairs_interest) against without, at 2,048 x 100 and
      2,048 x 256 (the ids of the uncapped top-100 / top-256),
  (e) miner_topk_merge_grouped at cap 3 against miner_topk_merge_capped (the stories, cap 1) and
      miner_topk_merge at 2,048 x (100 + 100).
Every interest-capped list is checked: its scores are the pair scores bit for bit, its interests the
pair form's, no interest more than cap times, and it equals the grouped post-hoc cap
(corpus.merge_topk(interest_cap=) with an empty first list) of the uncapped top-256 with its
interests wherever that fills the list. The parent library is recognised by having no
miner_rank_topk_interest symbol (the ABI number is the same). The two libraries' sizes are printed;
clean-build times are measured where they are built. The exit status is 0 only if every list of (b)
equals (a)'s, every (b) median lies inside (a)'s spread and every check of the new forms holds.
    python tools/rk_interest_ab.py PARENT_LIB [reps] [out.txt] [U] [N]"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from miner_amd import _lib, corpus, synthetic  # noqa: E402

dev = "cuda:0"
parent_path = sys.argv[1]
R = int(sys.argv[2]) if len(sys.argv) > 2 else 9
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
sub = torch.sort(torch.randperm(N, generator=g, device=dev)[:N // 20]).values.to(torch.int32).contiguous()   # 5 %
torch.cuda.synchronize()

parent = ctypes.CDLL(parent_path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # its own symbols, not this build's
for name in ("miner_rank_topk", "miner_rank_topk_filtered", "miner_rank_topk_subset", "miner_rank_topk_biased",
             "miner_rank_topk_capped", "miner_rank_topk_after"):
    getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
parent.miner_abi_version.restype = ctypes.c_int
lib = _lib.lib()
assert parent.miner_abi_version() == _lib.ABI_VERSION and not hasattr(parent, "miner_rank_topk_interest"), \
    "PARENT_LIB is not the parent commit's library"
F16, W = _lib.DTYPE_F16, _lib.SCORE_WEIGHTED
stream = lambda: torch.cuda.current_stream().cuda_stream
ptr = lambda x: None if x is None else x.data_ptr()
head = lambda: (stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K)

s0 = torch.empty(U, topk, dtype=torch.float32, device=dev)
i0 = torch.empty(U, topk, dtype=torch.int32, device=dev)
assert lib.miner_rank_topk(*head(), topk, ptr(s0), ptr(i0)) == 0
scale = float(s0.std())
bias = (scale * torch.randn((1, N), generator=g, device=dev)).contiguous()
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


def interest(cap, b=None):
    s, i = outs()
    gi = torch.empty(U, topk, dtype=torch.int32, device=dev)

    def run():
        rc = lib.miner_rank_topk_interest(*head(), topk, None, 0, None, None, -1, ptr(s), ptr(i), None, 0, ptr(b),
                                          0 if b is None else 1, None, None, 0, None, None, cap, ptr(gi))
        assert rc == 0, rc
        return s, i, gi
    return run


top256 = corpus.rank_topk(mui, proj, table, 256)
cand = {100: top256[1][:, :100].contiguous(), 256: top256[1]}


def pairs(C, with_interest):
    s = torch.empty(U, C, dtype=torch.float32, device=dev)
    gi = torch.empty(U, C, dtype=torch.int32, device=dev) if with_interest else None

    def run():
        rc = lib.miner_score_pairs_interest(*head(), ptr(cand[C]), C, ptr(s), None, 0, None, ptr(gi))
        assert rc == 0, rc
        return (s, gi) if with_interest else (s,)
    return run


ma = tuple(x.clone() for x in interest(3)())                         # two lists with interests to merge in (e)
mb = tuple(x.clone() for x in corpus.rank_topk(mui, proj, table, topk, news_ids=sub, return_interest=True))


def merged(kind):
    s, i = outs()
    gi = torch.empty(U, topk, dtype=torch.int32, device=dev)
    lists = lambda: (stream(), ptr(ma[0]), ptr(ma[1]), topk, ptr(mb[0]), ptr(mb[1]), topk, U, topk, None, 0, ptr(s), ptr(i))

    def run():
        if kind == "plain":
            rc = lib.miner_topk_merge(*lists())
        elif kind == "capped":
            rc = lib.miner_topk_merge_capped(*lists(), ptr(stories), N, 1)
        else:
            rc = lib.miner_topk_merge_grouped(*lists(), ptr(ma[2]), ptr(mb[2]), ptr(gi), 3)
        assert rc == 0, rc
        return (s, i, gi) if kind == "grouped" else (s, i)
    return run


FORMS = (("plain", plain), ("filtered", filtered), ("subset5", subset), ("biased", biased), ("capped", capped), ("cursor", cursor))
PAIRS = [(f"a_parent_{n}", f"b_{n}") for n, _ in FORMS]
VARIANTS = {}
for n, f in FORMS:
    VARIANTS[f"a_parent_{n}"], VARIANTS[f"b_{n}"] = f(parent), f(lib)
for cap in (1, 3, 10):
    VARIANTS[f"c_interest_cap{cap}"] = interest(cap)
for cap in (1, 3, 10):
    VARIANTS[f"c_interest_cap{cap}_biased"] = interest(cap, bias)
for C in (100, 256):
    VARIANTS[f"d_pairs_{C}"], VARIANTS[f"d_pairs_{C}_interest"] = pairs(C, False), pairs(C, True)
VARIANTS.update(e_merge=merged("plain"), e_merge_capped=merged("capped"), e_merge_grouped=merged("grouped"))


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


def interest_ok(lists, cap, b=None):
    """scores == the pair scores (+ prior) bit for bit, interests == the pair form's; no interest more
    than cap times; equal to the grouped post-hoc cap of the uncapped top-256 wherever that fills"""
    s, i, gi = lists
    kw = {} if b is None else dict(news_bias=b[0].contiguous())
    raw, rg = corpus.score_pairs(mui, proj, table, i, return_interest=True, **kw)
    same = torch.equal(bits(torch.where(i >= 0, raw, float("-inf"))), bits(s)) and torch.equal(rg, gi)
    c = torch.where(gi >= 0, gi, -1 - torch.arange(topk, device=dev, dtype=torch.int32)[None, :].expand_as(gi))
    cs = torch.sort(c, dim=1).values
    within = bool((cs[:, cap:] != cs[:, :-cap]).all()) if cap < topk else True
    top = corpus.rank_topk(mui, proj, table, 256, return_interest=True, **kw)
    post = corpus.merge_topk(tuple(x[:, :0] for x in top), top, topk, interest_cap=cap)
    filled = (post[1] >= 0).all(dim=1)
    prefix = all(torch.equal(bits(x[filled]), bits(y[filled])) for x, y in zip(post, lists))
    return same and within and prefix, float(filled.float().mean()), float((i >= 0).float().sum(dim=1).mean())


checks = {}
for cap in (1, 3, 10):
    checks[f"c_interest_cap{cap}"] = interest_ok(res[f"c_interest_cap{cap}"], cap)
    checks[f"c_interest_cap{cap}_biased"] = interest_ok(res[f"c_interest_cap{cap}_biased"], cap, bias)
d_ok = all(torch.equal(bits(res[f"d_pairs_{C}"][0]), bits(res[f"d_pairs_{C}_interest"][0])) for C in (100, 256))
e_ok = torch.equal(res["e_merge_grouped"][1], corpus.merge_topk(ma, mb, topk, interest_cap=3)[1])
share = torch.stack([(res["d_pairs_256_interest"][1] == k).sum(dim=1) for k in range(K)], dim=1).max(dim=1).values.float() / 256
med = {v: statistics.median(x) for v, x in ms.items()}
lines = [f"rk_interest_ab: U={U} N={N} L={L} K={K} d={d} fp16 weighted topk={topk}, {R} interleaved repeats, ms per call; "
         f"prior {scale:.4f} x randn [1, N]; stories: {int(stories.max()) + 1} clusters of 10, cap 1; subset: {sub.numel()} ids; "
         f"the most frequent interest holds {float(share.mean()):.3f} of a user's uncapped top-256 on average (max {float(share.max()):.3f})"]
for v in VARIANTS:
    x = ms[v]
    lines.append(f"{v:34s} median {med[v]:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}  "
                 f"spread {max(x) - min(x):6.3f}  all {[round(t, 3) for t in x]}")
gates, inside = [], []
for a_, b_ in PAIRS:
    diff = med[b_] - med[a_]
    spread = max(ms[a_]) - min(ms[a_])
    same = all(torch.equal(bits(x), bits(y)) for x, y in zip(res[a_], res[b_]))
    gates.append(same)
    inside.append(abs(diff) <= spread)
    lines.append(f"(b) - (a) {b_[2:]:9s}: {diff:+.3f} ms; (a)'s own spread {spread:.3f} ms -> "
                 f"{'within' if abs(diff) <= spread else 'OUTSIDE'} it; lists identical to (a): {same}")
for cap in (1, 3, 10):
    for suffix, base_ in (("", "b_filtered"), ("_biased", "b_biased")):
        v = f"c_interest_cap{cap}{suffix}"
        lines.append(f"(c) {v}: {med[v]:8.3f} ms = {med[v] / med['b_capped']:.3f} x b_capped ({med['b_capped']:.3f}) = "
                     f"{med[v] / med[base_]:.3f} x {base_} ({med[base_]:.3f}); exact, interests the pair form's, within cap, "
                     f"== grouped post-hoc cap of the top-256 where that fills: {checks[v][0]} (it fills for {checks[v][1]:.3f} of "
                     f"the users; {checks[v][2]:.1f} entries per list)")
for C in (100, 256):
    a_, b_ = f"d_pairs_{C}", f"d_pairs_{C}_interest"
    lines.append(f"(d) {U} x {C} pairs: {med[a_]:8.4f} ms, with interests {med[b_]:8.4f} ms = {med[b_] / med[a_]:.3f} x it")
lines.append(f"(d) the scores with and without interests are identical: {d_ok}")
lines.append(f"(e) {U} x ({topk} + {topk}): miner_topk_merge {med['e_merge']:8.4f} ms, capped {med['e_merge_capped']:8.4f} ms, "
             f"grouped (cap 3) {med['e_merge_grouped']:8.4f} ms = {med['e_merge_grouped'] / med['e_merge_capped']:.3f} x the capped "
             f"merge; equal to corpus.merge_topk(interest_cap=3): {e_ok}")
lines.append(f"library size: parent {os.path.getsize(parent_path)} bytes, this build {os.path.getsize(_lib.LIB_PATH)} bytes")
text = "\n".join(lines)
print(text, flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
# the exit status is the gate: identical lists AND every (b) median inside (a)'s own spread, then the new forms' checks
sys.exit(0 if all(gates) and all(inside) and all(c[0] for c in checks.values()) and d_ok and e_ok else 1)
