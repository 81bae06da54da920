"""Config-5 ranker step (2,048 users x 200,000 news, L = 200, K = 64, d = 768, fp16, top-100) in one
process, interleaved on the same inputs:
  (a) a library built from the parent commit (its miner_rank_topk_ws, loaded by path),
  (b) this build with no filters,
  (c) this build with exclude_history (E = 200) and a 50 % eligibility bitmap.
(b) must return (a)'s top-k bit for bit, and its median must lie within the spread (max - min) of
(a)'s own repeats; (c) is reported and checked against (b)'s list with the filtered ids struck out
of a deeper unfiltered list.
    python tools/rk_filter_ab.py PARENT_LIB [reps] [out.txt] [U] [N]"""
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
mask = torch.ones((U, L), dtype=torch.bool, device=dev)          # full histories: E = 200 real ids
elig = torch.rand((N,), generator=g, device=dev) < 0.5
W1, Q, W2 = synthetic.init_weights(5, d, Dc, K, device=dev)
pk = corpus.pack_encoder(W1, Q, W2, dtype=dt)
mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
seen = torch.where(mask, hid, torch.full_like(hid, -1))
words = corpus.pack_eligible(elig)
torch.cuda.synchronize()

parent = ctypes.CDLL(parent_path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # its own symbols, not this build's
res, args = _lib.SIGNATURES["miner_rank_topk_ws"]
parent.miner_rank_topk_ws.restype, parent.miner_rank_topk_ws.argtypes = res, args
parent.miner_rank_topk_workspace_bytes.restype = ctypes.c_size_t
parent.miner_rank_topk_split_recommended.restype = ctypes.c_int
parent.miner_abi_version.restype = ctypes.c_int
lib = _lib.lib()
assert parent.miner_abi_version() == _lib.ABI_VERSION - 1 and not hasattr(parent, "miner_rank_topk_filtered"), \
    "PARENT_LIB is not the parent commit's library"
nws_a = int(parent.miner_rank_topk_workspace_bytes(U, topk)) if parent.miner_rank_topk_split_recommended(U) else 0
ws_a = torch.empty(max(nws_a, 16), dtype=torch.uint8, device=dev)


def run_a():
    s = torch.empty(U, topk, dtype=torch.float32, device=dev)
    i = torch.empty(U, topk, dtype=torch.int32, device=dev)
    rc = parent.miner_rank_topk_ws(torch.cuda.current_stream().cuda_stream, _lib.DTYPE_F16, _lib.SCORE_WEIGHTED,
                                   mui.data_ptr(), proj.data_ptr(), table.data_ptr(), U, N, d, K, topk, s.data_ptr(),
                                   i.data_ptr(), ws_a.data_ptr() if nws_a else None, nws_a)
    assert rc == 0, rc
    return s, i


VARIANTS = {
    "a_parent": run_a,
    "b_unfiltered": lambda: corpus.rank_topk(mui, proj, table, topk),
    "c_filtered": lambda: corpus.rank_topk(mui, proj, table, topk, exclude_ids=seen, eligible=words),
}
ms, outs = {v: [] for v in VARIANTS}, {}
for v, fn in VARIANTS.items():                                     # warm-up, and the lists to compare
    outs[v] = tuple(x.clone() for x in fn())
torch.cuda.synchronize()
for _ in range(R):
    for v, fn in VARIANTS.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms[v].append(e0.elapsed_time(e1))

same_ab = torch.equal(outs["a_parent"][0], outs["b_unfiltered"][0]) and torch.equal(outs["a_parent"][1], outs["b_unfiltered"][1])
# (c) against the unfiltered top-256 with the filtered ids struck out, where 100 survivors remain in it
ds, di = corpus.rank_topk(mui, proj, table, 256)
keep = elig[di.long()] & ~(di[:, :, None] == seen[:, None, :]).any(-1)
enough = keep.sum(1) >= topk
pos = torch.where(keep, torch.cumsum(keep.int(), 1) - 1, torch.full_like(di, topk))
exp_i = torch.full((U, topk + 1), -1, dtype=torch.int32, device=dev).scatter_(1, pos.long().clamp(max=topk), di)[:, :topk]
same_c = bool((exp_i[enough] == outs["c_filtered"][1][enough]).all())
lines = [f"rk_filter_ab: U={U} N={N} L={L} K={K} d={d} fp16 top-{topk}, {R} interleaved repeats, ms per ranker step"]
for v in VARIANTS:
    x = ms[v]
    lines.append(f"{v:13s} median {statistics.median(x):8.3f}  min {min(x):8.3f}  max {max(x):8.3f}  "
                 f"spread {max(x) - min(x):6.3f}  all {[round(t, 3) for t in x]}")
diff = statistics.median(ms["b_unfiltered"]) - statistics.median(ms["a_parent"])
spread_a = max(ms["a_parent"]) - min(ms["a_parent"])
lines.append(f"(b) - (a) medians: {diff:+.3f} ms; (a)'s own spread {spread_a:.3f} ms -> "
             f"{'within' if abs(diff) <= spread_a else 'OUTSIDE'} it")
lines.append(f"(c) - (b) medians: {statistics.median(ms['c_filtered']) - statistics.median(ms['b_unfiltered']):+.3f} ms")
lines.append(f"(b) top-k identical to (a): {same_ab}; (c) equals the struck-out unfiltered top-256 "
             f"({int(enough.sum())} of {U} users with {topk} survivors in it): {same_c}")
text = "\n".join(lines)
print(text, flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
sys.exit(0 if same_ab and same_c else 1)
