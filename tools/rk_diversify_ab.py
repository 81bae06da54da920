"""The diversity re-ranking (miner_topk_diversify) beside the config-5 ranker step (2,048 users x
200,000 news, L = 200, K = 64, d = 768, fp16, weighted), in one process, interleaved on the same inputs:
  (a) the filtered rank step (a bitmap with every bit set, top-100) — the yardstick; its kernels are
      the parent commit's, compiled from unchanged sources — and the re-ranking of every user's
      ranked top-256 pool to 100 entries on the fp16 table: full pools, and half-empty pools (entries
      128 .. 255 turned into the (-inf, -1) tail, so the compaction leaves 4 of 8 tile rows),
  (b) the same pools on the fp32 and the bf16 copy of the table,
  (c) pools of P = 100 (the ranked top-100) re-ranked to 100.
The pools are real ranked lists (rank_topk, topk = 256), lambda = 0.7, relevance 'minmax'. Every
variant runs once per repeat in a fixed order; medians and spreads (max - min) over the repeats, and
each re-ranking's median as a ratio to the rank step's. Sanity only (the tests hold the yardstick):
every page is a subset of its pool without repeats and starts with the pool's best entry.
    python tools/rk_diversify_ab.py [reps] [out.txt] [U] [N] [LIB_BEFORE]
LIB_BEFORE: a library linked without diversify.o (or its size in bytes), for the size line."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from miner_amd import _lib, corpus, synthetic  # noqa: E402

dev = "cuda:0"
R = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else None
U = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
N = int(sys.argv[4]) if len(sys.argv) > 4 else 200000
before = sys.argv[5] if len(sys.argv) > 5 else None
L, K, d, Dc, topk, P, lam = 200, 64, 768, 200, 100, 256, 0.7
dt = torch.float16
g = torch.Generator(device=dev).manual_seed(5)
table = (torch.randn((N, d), generator=g, device=dev) / d ** 0.5).to(dt)
hid = torch.randint(0, N, (U, L), generator=g, device=dev, dtype=torch.int32)
mask = torch.ones((U, L), dtype=torch.bool, device=dev)
W1, Q, W2 = synthetic.init_weights(5, d, Dc, K, device=dev)
pk = corpus.pack_encoder(W1, Q, W2, dtype=dt)
mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
okw = corpus.pack_eligible(torch.ones(N, dtype=torch.bool, device=dev))
pool = tuple(x.contiguous() for x in corpus.rank_topk(mui, proj, table, P))
half = (pool[0].clone(), pool[1].clone())
half[0][:, P // 2:] = float("-inf")
half[1][:, P // 2:] = -1
p100 = (pool[0][:, :100].contiguous(), pool[1][:, :100].contiguous())
table32, table_bf = table.float(), table.to(torch.bfloat16)
torch.cuda.synchronize()


def rerank(lists, tab):
    return lambda: corpus.diversify_topk(lists, tab, topk, lam=lam, return_positions=True)


VARIANTS = {
    "a_rank_filtered": lambda: corpus.rank_topk(mui, proj, table, topk, eligible=okw),
    "a_diversify_fp16_full": rerank(pool, table),
    "a_diversify_fp16_half_empty": rerank(half, table),
    "b_diversify_fp32": rerank(pool, table32),
    "b_diversify_bf16": rerank(pool, table_bf),
    "c_diversify_fp16_P100": rerank(p100, table),
}
POOLS = {"a_diversify_fp16_full": pool, "a_diversify_fp16_half_empty": half, "b_diversify_fp32": pool,
         "b_diversify_bf16": pool, "c_diversify_fp16_P100": p100}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


ms, res = {v: [] for v in VARIANTS}, {}
for v, fn in VARIANTS.items():                                     # warm-up, and the results to look at
    res[v] = fn()
torch.cuda.synchronize()
for rep in range(R):
    for v, fn in VARIANTS.items():
        ms[v].append(timed(fn))


def sane(v):
    s, i, pos = res[v]
    ps, pi = POOLS[v]
    n = int((pi[0] >= 0).sum().clamp(max=topk))
    listed = pos[:, :n].long()
    subset = torch.equal(pi.gather(1, listed), i[:, :n]) and torch.equal(ps.gather(1, listed).view(torch.int32), s[:, :n].view(torch.int32))
    distinct = bool((torch.sort(listed, dim=1).values.diff(dim=1) > 0).all())
    first = bool((pos[:, 0] == 0).all())                           # rel = 1 and m = 0: the pool's best entry
    tail = bool((pos[:, n:] == -1).all() and (i[:, n:] == -1).all())
    moved = float((listed != torch.arange(n, device=dev)[None, :]).float().mean())
    return subset and distinct and first and tail, moved


med = {v: statistics.median(x) for v, x in ms.items()}
base = med["a_rank_filtered"]
lines = [f"rk_diversify_ab: U={U} N={N} L={L} K={K} d={d} weighted; pools = ranked top-{P} (fp16), re-ranked to {topk}, "
         f"lambda {lam}, minmax; {R} interleaved repeats, ms per call"]
oks = []
for v in VARIANTS:
    x = ms[v]
    line = (f"{v:30s} median {med[v]:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}  spread {max(x) - min(x):6.3f}  "
            f"= {med[v] / base:.4f} x the rank step")
    if v in POOLS:
        ok, moved = sane(v)
        oks.append(ok)
        line += f"; subset / distinct / best first / tail: {ok}; {moved:.3f} of the listed entries left their rank"
    lines.append(line + f"  all {[round(t, 3) for t in x]}")
size = f"library size: this build {os.path.getsize(_lib.LIB_PATH)} bytes"
if before:
    size += f", without diversify.o {int(before) if before.isdigit() else os.path.getsize(before)} bytes"
lines.append(size)
text = "\n".join(lines)
print(text, flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
sys.exit(0 if all(oks) else 1)
