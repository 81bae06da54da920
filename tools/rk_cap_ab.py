"""Config-5 ranker step (2,048 users x 200,000 news, L = 200, K = 64, d = 768, fp16, weighted, top-100)
in one process, interleaved on the same inputs:
  (a) a library built from the parent commit (loaded by path): its unfiltered, filtered (a bitmap
      with every bit set) and biased (G = 1) steps,
  (b) this build, the same three calls — each one's lists must equal (a)'s bit for bit and its median
      must lie within the spread (max - min) of (a)'s own repeats: the uncapped kernels are unchanged
      (each (a)/(b) pair swaps places every repeat),
  (c) this build's capped step (miner_rank_topk_capped) against the filtered step, and under the
      prior against the biased step, with 20,000 clusters of 10 news at cap 1 ("stories") and 300
      clusters at cap 3 ("publishers"), both assigned at random over the table,
  (d) the degenerate never-filling case at N = 8,192: 3 clusters, cap 2, top-100 — six entries per
      list, the threshold never rises and every step stages and merges all its 256 news — against
      the uncapped step at that N,
  (e) U = 256: the capped call (always unsplit) against the uncapped call in the split form the
      library recommends there — the price of having no split form under caps,
  (f) miner_topk_merge_capped against miner_topk_merge at 2,048 x (100 + 100).
Every capped list is checked: its scores are the uncapped pair scores bit for bit, no cluster more
than cap times, and it equals the post-hoc cap (corpus.cap_topk) of the uncapped top-256 wherever
that fills the list. The parent library is recognised by having no miner_rank_topk_capped symbol (the
ABI number is the same). The two libraries' sizes are printed; clean-build times are measured where
they are built.
    python tools/rk_cap_ab.py PARENT_LIB [reps] [out.txt] [U] [N]"""
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
ND, US = min(8192, N), min(256, U)                 # (d)'s table, (e)'s batch
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
three = (torch.arange(ND, device=dev) % 3).to(torch.int32)
torch.cuda.synchronize()

parent = ctypes.CDLL(parent_path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # its own symbols, not this build's
for name in ("miner_rank_topk", "miner_rank_topk_filtered", "miner_rank_topk_biased"):
    getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
parent.miner_abi_version.restype = ctypes.c_int
lib = _lib.lib()
assert parent.miner_abi_version() == _lib.ABI_VERSION and not hasattr(parent, "miner_rank_topk_capped"), \
    "PARENT_LIB is not the parent commit's library"
F16, W = _lib.DTYPE_F16, _lib.SCORE_WEIGHTED
stream = lambda: torch.cuda.current_stream().cuda_stream
ptr = lambda x: None if x is None else x.data_ptr()

s0 = torch.empty(U, topk, dtype=torch.float32, device=dev)
i0 = torch.empty(U, topk, dtype=torch.int32, device=dev)
assert lib.miner_rank_topk(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, topk, ptr(s0), ptr(i0)) == 0
scale = float(s0.std())
bias = (scale * torch.randn((1, N), generator=g, device=dev)).contiguous()


def outs(u=U, k=topk):
    return torch.empty(u, k, dtype=torch.float32, device=dev), torch.empty(u, k, dtype=torch.int32, device=dev)


def plain(handle):
    s, i = outs()

    def run():
        rc = handle.miner_rank_topk(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, topk, ptr(s), ptr(i))
        assert rc == 0, rc
        return s, i
    return run


def filtered(handle, u=U, n=N, ok=okw, ws=None):
    s, i = outs(u)

    def run():
        rc = handle.miner_rank_topk_filtered(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), u, n, d, K, topk, None, 0,
                                             ptr(ok), ptr(s), ptr(i), ptr(ws), 0 if ws is None else ws.numel())
        assert rc == 0, rc
        return s, i
    return run


def biased(handle):
    s, i = outs()

    def run():
        rc = handle.miner_rank_topk_biased(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, topk, None, 0, None,
                                           None, -1, ptr(s), ptr(i), None, 0, ptr(bias), 1, None)
        assert rc == 0, rc
        return s, i
    return run


def capped(clus, cap, b=None, u=U, n=N):
    s, i = outs(u)

    def run():
        rc = lib.miner_rank_topk_capped(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), u, n, d, K, topk, None, 0, None,
                                        None, -1, ptr(s), ptr(i), None, 0, ptr(b), 0 if b is None else 1, None, ptr(clus), cap)
        assert rc == 0, rc
        return s, i
    return run


nws = int(lib.miner_rank_topk_workspace_bytes(US, topk)) if lib.miner_rank_topk_split_recommended(US) else 0
ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
ma = tuple(x.clone() for x in capped(stories, 1)())                  # two capped lists to merge in (f)
mb = tuple(x.clone() for x in capped(publishers, 3)())


def merged(clus, cap):
    s, i = outs()

    def run():
        rc = lib.miner_topk_merge_capped(stream(), ptr(ma[0]), ptr(ma[1]), topk, ptr(mb[0]), ptr(mb[1]), topk, U, topk, None, 0,
                                         ptr(s), ptr(i), ptr(clus), 0 if clus is None else N, cap)
        assert rc == 0, rc
        return s, i
    return run


def merged_plain():
    s, i = outs()

    def run():
        rc = lib.miner_topk_merge(stream(), ptr(ma[0]), ptr(ma[1]), topk, ptr(mb[0]), ptr(mb[1]), topk, U, topk, None, 0,
                                  ptr(s), ptr(i))
        assert rc == 0, rc
        return s, i
    return run


PAIRS = [("a_parent_plain", "b_plain"), ("a_parent_filtered", "b_filtered"), ("a_parent_biased", "b_biased")]
VARIANTS = {
    "a_parent_plain": plain(parent), "b_plain": plain(lib),
    "a_parent_filtered": filtered(parent), "b_filtered": filtered(lib),
    "a_parent_biased": biased(parent), "b_biased": biased(lib),
    "c_capped_stories_cap1": capped(stories, 1), "c_capped_publishers_cap3": capped(publishers, 3),
    "c_capped_stories_cap1_biased": capped(stories, 1, bias), "c_capped_publishers_cap3_biased": capped(publishers, 3, bias),
    "d_uncapped_small": filtered(lib, n=ND, ok=None), "d_capped_degenerate": capped(three, 2, n=ND),
    "e_uncapped_small_batch": filtered(lib, u=US, ok=None, ws=ws), "e_capped_small_batch": capped(stories, 1, u=US),
    "f_merge": merged_plain(), "f_merge_capped": merged(stories, 1),
}


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


def capped_ok(lists, clus, cap, u=U, n=N, b=None, full=True):
    """scores == the uncapped pair scores (+ prior) bit for bit; no cluster more than cap times; equal
    to the post-hoc cap of the uncapped top-256 wherever that fills the list"""
    s, i = lists
    m, p_ = mui[:u], None if proj is None else proj[:u]
    kw = {} if b is None else dict(news_bias=b[0, :n].contiguous())
    raw = corpus.score_pairs(m, p_, table[:n], i, **kw)
    same = torch.equal(torch.where(i >= 0, raw, float("-inf")).view(torch.int32), s.view(torch.int32))
    c = torch.where(i >= 0, clus.long()[i.long().clamp(min=0)], -1)
    c = torch.where(c >= 0, c, -1 - torch.arange(topk, device=dev)[None, :].expand_as(c))     # unclustered: all distinct
    cs = torch.sort(c, dim=1).values
    within = bool((cs[:, cap:] != cs[:, :-cap]).all()) if cap < topk else True
    top = corpus.rank_topk(m, p_, table[:n], 256, **kw)
    post = corpus.cap_topk(top, clus, cap, topk)
    filled = (post[1] >= 0).all(dim=1)
    prefix = torch.equal(post[1][filled], i[filled]) and torch.equal(post[0][filled].view(torch.int32), s[filled].view(torch.int32))
    return same and within and prefix and (bool(filled.any()) or not full), float(filled.float().mean())


checks = {
    "c_capped_stories_cap1": capped_ok(res["c_capped_stories_cap1"], stories, 1),
    "c_capped_publishers_cap3": capped_ok(res["c_capped_publishers_cap3"], publishers, 3),
    "c_capped_stories_cap1_biased": capped_ok(res["c_capped_stories_cap1_biased"], stories, 1, b=bias),
    "c_capped_publishers_cap3_biased": capped_ok(res["c_capped_publishers_cap3_biased"], publishers, 3, b=bias),
    "d_capped_degenerate": capped_ok(res["d_capped_degenerate"], three, 2, n=ND, full=False),
    "e_capped_small_batch": capped_ok(res["e_capped_small_batch"], stories, 1, u=US),
}
six = bool(((res["d_capped_degenerate"][1] >= 0).sum(dim=1) == 6).all())
e_same = torch.equal(res["e_capped_small_batch"][1], res["c_capped_stories_cap1"][1][:US])
in_b = ((ma[1][:, :, None] == mb[1][:, None, :]) & (ma[1][:, :, None] >= 0)).any(dim=2)   # b's entry replaces a's
f_want = corpus.cap_topk((torch.cat([ma[0], mb[0]], dim=1), torch.cat([torch.where(in_b, -1, ma[1]), mb[1]], dim=1)),
                         stories, 1, topk)
med = {v: statistics.median(x) for v, x in ms.items()}
lines = [f"rk_cap_ab: U={U} N={N} L={L} K={K} d={d} fp16 weighted topk={topk}, {R} interleaved repeats, ms per call; "
         f"prior {scale:.4f} x randn [1, N]; stories: {int(stories.max()) + 1} clusters of 10, cap 1; publishers: 300 clusters, cap 3"]
for v in VARIANTS:
    x = ms[v]
    lines.append(f"{v:34s} median {med[v]:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}  "
                 f"spread {max(x) - min(x):6.3f}  all {[round(t, 3) for t in x]}")
gates = []
for a_, b_ in PAIRS:
    diff = med[b_] - med[a_]
    spread = max(ms[a_]) - min(ms[a_])
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(res[a_], res[b_]))
    gates.append(same)
    lines.append(f"(b) - (a) {b_[2:]:9s}: {diff:+.3f} ms; (a)'s own spread {spread:.3f} ms -> "
                 f"{'within' if abs(diff) <= spread else 'OUTSIDE'} it; lists identical to (a): {same}")
for v, base_ in (("c_capped_stories_cap1", "b_filtered"), ("c_capped_publishers_cap3", "b_filtered"),
                 ("c_capped_stories_cap1_biased", "b_biased"), ("c_capped_publishers_cap3_biased", "b_biased")):
    lines.append(f"(c) {v}: {med[v]:8.3f} ms = {med[v] / med[base_]:.3f} x {base_} ({med[base_]:.3f}); exact, within cap, "
                 f"== post-hoc cap of the top-256 where that fills: {checks[v][0]} (it fills for {checks[v][1]:.3f} of the users)")
lines.append(f"(d) N={ND}, 3 clusters, cap 2: capped {med['d_capped_degenerate']:8.3f} ms = "
             f"{med['d_capped_degenerate'] / med['d_uncapped_small']:.3f} x the uncapped step at that N "
             f"({med['d_uncapped_small']:.3f}); six entries per list: {six}; checks: {checks['d_capped_degenerate'][0]}")
lines.append(f"(e) U={US}: capped (unsplit) {med['e_capped_small_batch']:8.3f} ms = "
             f"{med['e_capped_small_batch'] / med['e_uncapped_small_batch']:.3f} x the uncapped call "
             f"({'split form' if nws else 'unsplit: no split form on this device'}, {med['e_uncapped_small_batch']:.3f}); "
             f"checks: {checks['e_capped_small_batch'][0]}; the same lists as in the full batch: {e_same}")
f_ok = torch.equal(f_want[1], res["f_merge_capped"][1]) and \
    torch.equal(f_want[0].view(torch.int32), res["f_merge_capped"][0].view(torch.int32))
lines.append(f"(f) {U} x ({topk} + {topk}): miner_topk_merge {med['f_merge']:8.4f} ms, capped {med['f_merge_capped']:8.4f} ms = "
             f"{med['f_merge_capped'] / med['f_merge']:.3f} x it; equal to the cap of the two lists side by side: {f_ok}")
lines.append(f"library size: parent {os.path.getsize(parent_path)} bytes, this build {os.path.getsize(_lib.LIB_PATH)} bytes")
text = "\n".join(lines)
print(text, flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
sys.exit(0 if all(gates) and all(c[0] for c in checks.values()) and six and e_same and f_ok else 1)
