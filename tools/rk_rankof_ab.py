"""Config-5 ranker step (2,048 users x 200,000 news, L = 200, K = 64, d = 768, fp16, weighted) in one
process, interleaved on the same inputs:
  (a) a library built from the parent commit (loaded by path): its miner_rank_topk at topk = 100,
  (b) this build, the same call — its lists must equal (a)'s bit for bit and its median must lie
      within the spread (max - min) of (a)'s own repeats: the existing kernels are unchanged
      ((a) and (b) swap places every repeat, so neither always runs behind the other),
  (c) this build's counting form (miner_rank_count) at T = 1 / 8 / 64, without and with a bitmap
      (a random 60 % of the table) — the targets are the first T entries of (b)'s lists with their
      scores, so without a bitmap counts[u, j] must be j exactly; ms per call and the ratio to (a),
  (d) this build's pair form (miner_score_pairs) at C = 100 (the ids of (b)'s lists: the scores
      must equal the lists' bit for bit) and C = 256 (random ids).
The parent library is recognised by having no miner_score_pairs symbol (the ABI number is the
same). The two libraries' sizes are printed; clean-build times are measured where they are built.
    python tools/rk_rankof_ab.py PARENT_LIB [reps] [out.txt] [U] [N]"""
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
TS, CS = (1, 8, 64), (100, 256)
dt = torch.float16
g = torch.Generator(device=dev).manual_seed(5)
table = (torch.randn((N, d), generator=g, device=dev) / d ** 0.5).to(dt)
hid = torch.randint(0, N, (U, L), generator=g, device=dev, dtype=torch.int32)
mask = torch.ones((U, L), dtype=torch.bool, device=dev)
W1, Q, W2 = synthetic.init_weights(5, d, Dc, K, device=dev)
pk = corpus.pack_encoder(W1, Q, W2, dtype=dt)
mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
okw = corpus.pack_eligible(torch.rand(N, generator=g, device=dev) < 0.6)
rand_ids = torch.randint(0, N, (U, 256), generator=g, device=dev, dtype=torch.int32)
torch.cuda.synchronize()

parent = ctypes.CDLL(parent_path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # its own symbols, not this build's
parent.miner_rank_topk.restype, parent.miner_rank_topk.argtypes = _lib.SIGNATURES["miner_rank_topk"]
parent.miner_abi_version.restype = ctypes.c_int
lib = _lib.lib()
assert parent.miner_abi_version() == _lib.ABI_VERSION and not hasattr(parent, "miner_score_pairs"), \
    "PARENT_LIB is not the parent commit's library"
F16, W = _lib.DTYPE_F16, _lib.SCORE_WEIGHTED
stream = lambda: torch.cuda.current_stream().cuda_stream


def rank(handle):
    s = torch.empty(U, topk, dtype=torch.float32, device=dev)
    i = torch.empty(U, topk, dtype=torch.int32, device=dev)
    rc = handle.miner_rank_topk(stream(), F16, W, mui.data_ptr(), proj.data_ptr(), table.data_ptr(), U, N, d, K, topk,
                                s.data_ptr(), i.data_ptr())
    assert rc == 0, rc
    return s, i


top_s, top_i = rank(lib)
torch.cuda.synchronize()


def count(T, words):
    ts, ti = top_s[:, :T].contiguous(), top_i[:, :T].contiguous()
    out = torch.empty(U, T, dtype=torch.int32, device=dev)

    def run():
        rc = lib.miner_rank_count(stream(), F16, W, mui.data_ptr(), proj.data_ptr(), table.data_ptr(), U, N, d, K,
                                  ts.data_ptr(), ti.data_ptr(), T, None if words is None else words.data_ptr(), out.data_ptr())
        assert rc == 0, rc
        return (out,)
    return run


def pairs(ids):
    C = ids.shape[1]
    out = torch.empty(U, C, dtype=torch.float32, device=dev)

    def run():
        rc = lib.miner_score_pairs(stream(), F16, W, mui.data_ptr(), proj.data_ptr(), table.data_ptr(), U, N, d, K,
                                   ids.data_ptr(), C, out.data_ptr())
        assert rc == 0, rc
        return (out,)
    return run


VARIANTS = {"a_parent_rank_topk": lambda: rank(parent), "b_rank_topk": lambda: rank(lib)}
for T in TS:
    VARIANTS[f"c_count_T{T}"] = count(T, None)
    VARIANTS[f"c_count_T{T}_bitmap"] = count(T, okw)
VARIANTS["d_pairs_C100"] = pairs(top_i.contiguous())
VARIANTS["d_pairs_C256"] = pairs(rand_ids)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


ms, outs = {v: [] for v in VARIANTS}, {}
for v, fn in VARIANTS.items():                                     # warm-up, and the results to compare
    outs[v] = tuple(x.clone() for x in fn())
torch.cuda.synchronize()
names = list(VARIANTS)
for rep in range(R):
    # the gate pair swaps places every repeat: the same code must not be told apart by what ran before it
    order = names if rep % 2 == 0 else [names[1], names[0]] + names[2:]
    for v in order:
        ms[v].append(timed(VARIANTS[v]))

same_ab = all(torch.equal(x, y) for x, y in zip(outs["a_parent_rank_topk"], outs["b_rank_topk"]))
exact_c = {T: torch.equal(outs[f"c_count_T{T}"][0], torch.arange(T, dtype=torch.int32, device=dev).expand(U, T)) for T in TS}
below_c = {T: bool((outs[f"c_count_T{T}_bitmap"][0] <= outs[f"c_count_T{T}"][0]).all()) for T in TS}
same_d = torch.equal(outs["d_pairs_C100"][0].view(torch.int32), top_s.view(torch.int32))
med = {v: statistics.median(x) for v, x in ms.items()}
a = med["a_parent_rank_topk"]
lines = [f"rk_rankof_ab: U={U} N={N} L={L} K={K} d={d} fp16 weighted, {R} interleaved repeats, ms per call; "
         f"(a), (b): miner_rank_topk at topk={topk}"]
for v in VARIANTS:
    x = ms[v]
    lines.append(f"{v:20s} median {med[v]:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}  "
                 f"spread {max(x) - min(x):6.3f}  all {[round(t, 3) for t in x]}")
diff = med["b_rank_topk"] - a
spread_a = max(ms["a_parent_rank_topk"]) - min(ms["a_parent_rank_topk"])
gate = abs(diff) <= spread_a
lines.append(f"(b) - (a) medians: {diff:+.3f} ms; (a)'s own spread {spread_a:.3f} ms -> "
             f"{'within' if gate else 'OUTSIDE'} it; (b) lists identical to (a): {same_ab}")
for T in TS:
    c, cb = med[f"c_count_T{T}"], med[f"c_count_T{T}_bitmap"]
    lines.append(f"(c) T={T:2d}: counting form {c:8.3f} ms = {c / a:.3f} x (a), with a bitmap {cb:8.3f} ms = {cb / a:.3f} x (a); "
                 f"counts[u, j] == j: {exact_c[T]}; with the bitmap never more: {below_c[T]}")
c1, c64 = med["c_count_T1"], med["c_count_T64"]
lines.append(f"(c) T=64 - T=1: {c64 - c1:+.3f} ms = {(c64 - c1) / a:.3f} x (a) "
             f"({'more' if c64 > c1 + a / 2 else 'not more'} than the T=1 line plus half of (a))")
for C in CS:
    p = med[f"d_pairs_C{C}"]
    lines.append(f"(d) C={C}: pair form {p:8.3f} ms = {p / a:.4f} x (a), {1e6 * p / (U * C):.1f} ns per pair"
                 + (f"; scores identical to (b)'s lists: {same_d}" if C == topk else ""))
lines.append(f"library size: parent {os.path.getsize(parent_path)} bytes, this build {os.path.getsize(_lib.LIB_PATH)} bytes")
text = "\n".join(lines)
print(text, flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
sys.exit(0 if same_ab and all(exact_c.values()) and all(below_c.values()) and same_d else 1)
