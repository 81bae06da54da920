"""Config-5 ranker step (2,048 users x 200,000 news, L = 200, K = 64, d = 768, fp16, weighted, top-100)
in one process, interleaved on the same inputs:
  (a) a library built from the parent commit (loaded by path): its unfiltered, filtered (a bitmap
      with every bit set), subset (5 % of the table), biased (G = 1) and capped (20,000 clusters of
      10 news, cap 1) steps,
  (b) this build, the same five calls without a cursor — each one's lists must equal (a)'s bit for
      bit and its median must lie within the spread (max - min) of (a)'s own repeats: the kernels a
      call without a cursor launches are the code they were, or cost what they did (each (a)/(b)
      pair swaps places every repeat),
  (c) this build's cursor step (miner_rank_topk_after, no filter) at page 2 — each user's 100th entry
      as its cursor — against the filtered step,
  (d) the cursor step at a deep cursor: a random news per user, its miner_score_pairs score and its
      id (mean depth about N / 2: most entries that pass the threshold test are turned away by the
      cursor) against the filtered step,
  (e) U = 256: the cursor step (page 2) in the split form the library recommends there, against the
      split form without a cursor,
  (f) corpus.rank_topk_deep at topk = 1,000 (four pages) against 4 x the page-1 step.
Every cursor list is checked: page 1 + page 2 is the top-200 list bit for bit; the deep cursor's
page holds, per user, the news whose exact rank (corpus.rank_of, the counting form) is the cursor
news' rank + 1 + j; the deep list begins with the top-256 list and rank_of of its column j is j. The
parent library is recognised by having no miner_rank_topk_after symbol (the ABI number is the same).
The two libraries' sizes are printed; clean-build times are measured where they are built.
    python tools/rk_after_ab.py PARENT_LIB [reps] [out.txt] [U] [N]"""
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
US = min(256, U)                                   # (e)'s batch
DEEP = 1000                                        # (f)'s depth
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
sub = corpus.canonical_news_ids(torch.randperm(N, generator=g, device=dev)[:N // 20], N).ids
MS = sub.numel()
torch.cuda.synchronize()

parent = ctypes.CDLL(parent_path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # its own symbols, not this build's
for name in ("miner_rank_topk", "miner_rank_topk_filtered", "miner_rank_topk_subset", "miner_rank_topk_biased",
             "miner_rank_topk_capped"):
    getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
parent.miner_abi_version.restype = ctypes.c_int
lib = _lib.lib()
assert parent.miner_abi_version() == _lib.ABI_VERSION and not hasattr(parent, "miner_rank_topk_after"), \
    "PARENT_LIB is not the parent commit's library"
F16, W = _lib.DTYPE_F16, _lib.SCORE_WEIGHTED
stream = lambda: torch.cuda.current_stream().cuda_stream
ptr = lambda x: None if x is None else x.data_ptr()

s0 = torch.empty(U, topk, dtype=torch.float32, device=dev)
i0 = torch.empty(U, topk, dtype=torch.int32, device=dev)
assert lib.miner_rank_topk(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, topk, ptr(s0), ptr(i0)) == 0
scale = float(s0.std())
bias = (scale * torch.randn((1, N), generator=g, device=dev)).contiguous()
# the cursors: page 2 (each user's 100th entry), and a random news per user with its pair score
page2_cur = (s0[:, -1].contiguous(), i0[:, -1].contiguous())
deep_i = torch.randint(0, N, (U,), generator=g, device=dev, dtype=torch.int32)
deep_cur = (corpus.score_pairs(mui, proj, table, deep_i[:, None])[:, 0].contiguous(), deep_i)
torch.cuda.synchronize()


def outs(u=U, k=topk):
    return torch.empty(u, k, dtype=torch.float32, device=dev), torch.empty(u, k, dtype=torch.int32, device=dev)


def plain(handle):
    s, i = outs()

    def run():
        rc = handle.miner_rank_topk(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, topk, ptr(s), ptr(i))
        assert rc == 0, rc
        return s, i
    return run


def filtered(handle, u=U, ok=okw, ws=None):
    s, i = outs(u)

    def run():
        rc = handle.miner_rank_topk_filtered(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), u, N, d, K, topk, None, 0,
                                             ptr(ok), ptr(s), ptr(i), ptr(ws), 0 if ws is None else ws.numel())
        assert rc == 0, rc
        return s, i
    return run


def subset(handle):
    s, i = outs()

    def run():
        rc = handle.miner_rank_topk_subset(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, topk, None, 0, None,
                                           ptr(sub), MS, ptr(s), ptr(i), None, 0)
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


def capped(handle):
    s, i = outs()

    def run():
        rc = handle.miner_rank_topk_capped(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, topk, None, 0, None,
                                           None, -1, ptr(s), ptr(i), None, 0, None, 0, None, ptr(stories), 1)
        assert rc == 0, rc
        return s, i
    return run


def cursor(cur, u=U, ws=None):
    s, i = outs(u)

    def run():
        rc = lib.miner_rank_topk_after(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), u, N, d, K, topk, None, 0, None,
                                       None, -1, ptr(s), ptr(i), ptr(ws), 0 if ws is None else ws.numel(), None, 0, None,
                                       None, 0, ptr(cur[0]), ptr(cur[1]))
        assert rc == 0, rc
        return s, i
    return run


def deep():
    return corpus.rank_topk_deep(mui, proj, table, DEEP)


nws = int(lib.miner_rank_topk_workspace_bytes(US, topk)) if lib.miner_rank_topk_split_recommended(US) else 0
ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
os.environ.pop("MINER_RK_SPLIT", None)             # (f) takes the form the library recommends at U

PAIRS = [("a_parent_plain", "b_plain"), ("a_parent_filtered", "b_filtered"), ("a_parent_subset5", "b_subset5"),
         ("a_parent_biased", "b_biased"), ("a_parent_capped", "b_capped")]
VARIANTS = {
    "a_parent_plain": plain(parent), "b_plain": plain(lib),
    "a_parent_filtered": filtered(parent), "b_filtered": filtered(lib),
    "a_parent_subset5": subset(parent), "b_subset5": subset(lib),
    "a_parent_biased": biased(parent), "b_biased": biased(lib),
    "a_parent_capped": capped(parent), "b_capped": capped(lib),
    "c_cursor_page2": cursor(page2_cur), "d_cursor_deep": cursor(deep_cur),
    "e_small_batch": filtered(lib, u=US, ok=None, ws=ws), "e_small_batch_cursor_page2": cursor(page2_cur, u=US, ws=ws),
    "f_deep_1000": deep,
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


def eq(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


# the cursor lists
top200 = corpus.rank_topk(mui, proj, table, 2 * topk)
c_ok = eq((torch.cat([res["b_plain"][0], res["c_cursor_page2"][0]], 1), torch.cat([res["b_plain"][1], res["c_cursor_page2"][1]], 1)),
          top200)
e_ok = eq(res["e_small_batch_cursor_page2"], (res["c_cursor_page2"][0][:US], res["c_cursor_page2"][1][:US]))
cols = torch.arange(64, device=dev)
r_cur = corpus.rank_of(mui, proj, table, deep_i[:, None])[0].long()
r_page, s_page = corpus.rank_of(mui, proj, table, res["d_cursor_deep"][1][:, :64])
listed = res["d_cursor_deep"][1][:, :64] >= 0
d_ok = bool((torch.where(listed, r_page.long(), r_cur + 1 + cols[None, :]) == r_cur + 1 + cols[None, :]).all()) and \
    bool((listed.sum(dim=1) == (N - 1 - r_cur[:, 0]).clamp(max=64)).all()) and \
    torch.equal(torch.where(listed, s_page, float("-inf")).view(torch.int32), res["d_cursor_deep"][0][:, :64].contiguous().view(torch.int32))
depth = float(r_cur.float().mean())
top256 = corpus.rank_topk(mui, proj, table, 256)
pick = torch.linspace(0, DEEP - 1, 64, device=dev).long()
f_ok = eq((res["f_deep_1000"][0][:, :256], res["f_deep_1000"][1][:, :256]), top256) and \
    torch.equal(corpus.rank_of(mui, proj, table, res["f_deep_1000"][1][:, pick].contiguous())[0].long(), pick[None, :].expand(U, 64))

med = {v: statistics.median(x) for v, x in ms.items()}
lines = [f"rk_after_ab: U={U} N={N} L={L} K={K} d={d} fp16 weighted topk={topk}, {R} interleaved repeats, ms per call; "
         f"subset: {MS} ids; prior {scale:.4f} x randn [1, N]; stories: {int(stories.max()) + 1} clusters of 10, cap 1"]
for v in VARIANTS:
    x = ms[v]
    lines.append(f"{v:34s} median {med[v]:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}  "
                 f"spread {max(x) - min(x):6.3f}  all {[round(t, 3) for t in x]}")
gates, inside = [], []
for a_, b_ in PAIRS:
    diff = med[b_] - med[a_]
    spread = max(ms[a_]) - min(ms[a_])
    same = eq(res[a_], res[b_])
    gates.append(same)
    inside.append(abs(diff) <= spread)
    lines.append(f"(b) - (a) {b_[2:]:9s}: {diff:+.3f} ms; (a)'s own spread {spread:.3f} ms -> "
                 f"{'within' if abs(diff) <= spread else 'OUTSIDE'} it; lists identical to (a): {same}")
lines.append(f"(c) cursor step, page 2 (each user's 100th entry): {med['c_cursor_page2']:8.3f} ms = "
             f"{med['c_cursor_page2'] / med['b_filtered']:.3f} x b_filtered ({med['b_filtered']:.3f}); "
             f"page 1 + page 2 == the top-200 list bit for bit: {c_ok}")
lines.append(f"(d) cursor step, deep cursor (a random news per user, mean rank {depth:.0f} of {N}): {med['d_cursor_deep']:8.3f} ms = "
             f"{med['d_cursor_deep'] / med['b_filtered']:.3f} x b_filtered; rank_of(page[j]) == rank_of(cursor) + 1 + j, scores "
             f"bit for bit: {d_ok}")
lines.append(f"(e) U={US} ({'split form' if nws else 'unsplit: no split form on this device'}): cursor step, page 2 "
             f"{med['e_small_batch_cursor_page2']:8.3f} ms = {med['e_small_batch_cursor_page2'] / med['e_small_batch']:.3f} x the "
             f"step without a cursor ({med['e_small_batch']:.3f}); the same lists as in the full batch: {e_ok}")
lines.append(f"(f) rank_topk_deep, topk = {DEEP} ({-(-DEEP // 256)} pages): {med['f_deep_1000']:8.3f} ms = "
             f"{med['f_deep_1000'] / (4 * med['b_plain']):.3f} x (4 x b_plain = {4 * med['b_plain']:.3f}); begins with the top-256 "
             f"list, rank_of(column j) == j at 64 columns: {f_ok}")
lines.append(f"library size: parent {os.path.getsize(parent_path)} bytes, this build {os.path.getsize(_lib.LIB_PATH)} bytes")
text = "\n".join(lines)
print(text, flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
sys.exit(0 if all(gates) and c_ok and d_ok and e_ok and f_ok else 1)
