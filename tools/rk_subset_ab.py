"""Config-5 ranker step (2,048 users x 200,000 news, L = 200, K = 64, d = 768, fp16, top-100) in one
process, interleaved on the same inputs:
  (a) a library built from the parent commit (loaded by path): its miner_rank_topk_filtered with the
      bitmap of M = 10,000 ids,
  (b) this build, the same call — its lists must equal (a)'s bit for bit and its median must lie
      within the spread (max - min) of (a)'s own repeats: the existing kernels are unchanged,
  (c) this build's subset form (miner_rank_topk_subset) at M = 2,000 / 10,000 / 50,000 / 200,000 —
      each list must equal this build's bitmap form for the same set bit for bit; ms per M and the
      ratio to (a),
  (d) miner_topk_merge on 2,048 x (100 + 100).
The parent library is recognised by having no miner_rank_topk_subset symbol (the ABI number is the
same). The bitmap form's time at the other M values is taken once, outside the interleaved loop, for
the break-even estimate.
    python tools/rk_subset_ab.py PARENT_LIB [reps] [out.txt] [U] [N]"""
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
MS = [m for m in (2000, 10000, 50000, 200000) if m <= N] if N == 200000 else sorted({max(1, N // 100), N // 20, N // 4, N})
M_AB = 10000 if N == 200000 else N // 20
dt = torch.float16
g = torch.Generator(device=dev).manual_seed(5)
table = (torch.randn((N, d), generator=g, device=dev) / d ** 0.5).to(dt)
hid = torch.randint(0, N, (U, L), generator=g, device=dev, dtype=torch.int32)
mask = torch.ones((U, L), dtype=torch.bool, device=dev)
W1, Q, W2 = synthetic.init_weights(5, d, Dc, K, device=dev)
pk = corpus.pack_encoder(W1, Q, W2, dtype=dt)
mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
perm = torch.randperm(N, generator=g, device=dev)
id_lists = {m: corpus.canonical_news_ids(perm[:m], N) for m in MS}            # sorted, distinct: canonicalised once
words = {}
for m in MS:
    member = torch.zeros(N, dtype=torch.bool, device=dev)
    member[id_lists[m].ids.long()] = True
    words[m] = corpus.pack_eligible(member)
torch.cuda.synchronize()

parent = ctypes.CDLL(parent_path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # its own symbols, not this build's
res, args = _lib.SIGNATURES["miner_rank_topk_filtered"]
parent.miner_rank_topk_filtered.restype, parent.miner_rank_topk_filtered.argtypes = res, args
parent.miner_rank_topk_workspace_bytes.restype = ctypes.c_size_t
parent.miner_rank_topk_split_recommended.restype = ctypes.c_int
parent.miner_abi_version.restype = ctypes.c_int
lib = _lib.lib()
assert parent.miner_abi_version() == _lib.ABI_VERSION and not hasattr(parent, "miner_rank_topk_subset"), \
    "PARENT_LIB is not the parent commit's library"
nws_a = int(parent.miner_rank_topk_workspace_bytes(U, topk)) if parent.miner_rank_topk_split_recommended(U) else 0
ws_a = torch.empty(max(nws_a, 16), dtype=torch.uint8, device=dev)


def run_a():
    s = torch.empty(U, topk, dtype=torch.float32, device=dev)
    i = torch.empty(U, topk, dtype=torch.int32, device=dev)
    rc = parent.miner_rank_topk_filtered(torch.cuda.current_stream().cuda_stream, _lib.DTYPE_F16, _lib.SCORE_WEIGHTED,
                                         mui.data_ptr(), proj.data_ptr(), table.data_ptr(), U, N, d, K, topk, None, 0,
                                         words[M_AB].data_ptr(), s.data_ptr(), i.data_ptr(),
                                         ws_a.data_ptr() if nws_a else None, nws_a)
    assert rc == 0, rc
    return s, i


la = corpus.rank_topk(mui, proj, table, topk, news_ids=id_lists[M_AB])
lb = corpus.rank_topk(mui, proj, table, topk, news_ids=id_lists[MS[0]])
torch.cuda.synchronize()

VARIANTS = {"a_parent_bitmap": run_a,
            "b_bitmap": lambda: corpus.rank_topk(mui, proj, table, topk, eligible=words[M_AB])}
for m in MS:
    VARIANTS[f"c_subset_{m}"] = (lambda m: lambda: corpus.rank_topk(mui, proj, table, topk, news_ids=id_lists[m]))(m)
VARIANTS["d_topk_merge"] = lambda: corpus.merge_topk(la, lb, topk)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


ms, outs = {v: [] for v in VARIANTS}, {}
for v, fn in VARIANTS.items():                                     # warm-up, and the lists to compare
    outs[v] = tuple(x.clone() for x in fn())
torch.cuda.synchronize()
for _ in range(R):
    for v, fn in VARIANTS.items():
        ms[v].append(timed(fn))

eq = lambda x, y: torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
same_ab = eq(outs["a_parent_bitmap"], outs["b_bitmap"])
bitmap_ms, same_c = {}, {}
for m in MS:                                                        # this build's bitmap form per set: the list, one timing
    fn = lambda: corpus.rank_topk(mui, proj, table, topk, eligible=words[m])
    want = tuple(x.clone() for x in fn())
    bitmap_ms[m] = statistics.median(timed(fn) for _ in range(3))
    same_c[m] = eq(outs[f"c_subset_{m}"], want)
med = {v: statistics.median(x) for v, x in ms.items()}
lines = [f"rk_subset_ab: U={U} N={N} L={L} K={K} d={d} fp16 top-{topk}, {R} interleaved repeats, ms per call; "
         f"(a), (b): the bitmap of M={M_AB} ids"]
for v in VARIANTS:
    x = ms[v]
    lines.append(f"{v:17s} median {med[v]:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}  "
                 f"spread {max(x) - min(x):6.3f}  all {[round(t, 3) for t in x]}")
diff = med["b_bitmap"] - med["a_parent_bitmap"]
spread_a = max(ms["a_parent_bitmap"]) - min(ms["a_parent_bitmap"])
lines.append(f"(b) - (a) medians: {diff:+.3f} ms; (a)'s own spread {spread_a:.3f} ms -> "
             f"{'within' if abs(diff) <= spread_a else 'OUTSIDE'} it; (b) lists identical to (a): {same_ab}")
for m in MS:
    c = med[f"c_subset_{m}"]
    lines.append(f"(c) M={m:7d} ({100.0 * m / N:5.1f} % of N): subset {c:8.3f} ms = {c / med['a_parent_bitmap']:.3f} x (a); "
                 f"bitmap form for the same set {bitmap_ms[m]:8.3f} ms (3 repeats); lists identical: {same_c[m]}")
# break-even share: where the subset form's time (linear between the measured M) meets the bitmap form's
pts = [(m, med[f"c_subset_{m}"], bitmap_ms[m]) for m in MS]
be = None
for (m0, c0, b0), (m1, c1, b1) in zip(pts, pts[1:]):
    if c0 <= b0 and c1 > b1:
        f = (b0 - c0) / ((b0 - c0) + (c1 - b1))
        be = (m0 + f * (m1 - m0)) / N
if be is not None:
    lines.append(f"break-even: the bitmap form is the faster one above M/N = {be:.2f} (linear between the measured M)")
elif pts[0][1] > pts[0][2]:
    lines.append("break-even: the subset form is not faster than the bitmap form at any measured M")
else:
    lines.append("break-even: the subset form is at least as fast as the bitmap form at every measured M, M = N included")
lines.append(f"(d) topk_merge {U} x ({topk} + {topk}) -> {topk}: median {med['d_topk_merge']:.3f} ms")
text = "\n".join(lines)
print(text, flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
sys.exit(0 if same_ab and all(same_c.values()) else 1)
