"""Config-5 ranker step (2,048 users x 200,000 news, L = 200, K = 64, d = 768, fp16, weighted) in one
process, interleaved on the same inputs:
  (a) a library built from the parent commit (loaded by path): its miner_rank_topk at topk = 100,
  (b) this build, the same call — its lists must equal (a)'s bit for bit and its median must lie
      within the spread (max - min) of (a)'s own repeats: the unbiased kernels are unchanged
      ((a) and (b) swap places every repeat, so neither always runs behind the other),
  (c) this build's biased top-k (miner_rank_topk_biased), table form, with G = 1 and with G = 4
      (user u in group u % 4: the two users of a tile read different rows), and the subset form at
      5 % of the table against the unbiased subset call on the same ids,
  (d) the biased counting form (miner_rank_count_biased) at T = 1 and T = 64 against the unbiased
      one — the targets are the first T entries of the biased lists with their scores, so
      counts[u, j] must be j exactly,
  (e) the biased pair form (miner_score_pairs_biased) at C = 100 on the ids of the biased lists: the
      scores must equal the lists' bit for bit.
Every biased list is also checked against the unbiased pair scores plus the prior in torch fp32
(one IEEE add): the listed score of (u, n) must be score_pairs(u, n) + bias[group(u), n] bit for bit.
The parent library is recognised by having no miner_rank_topk_biased symbol (the ABI number is the
same). The two libraries' sizes are printed; clean-build times are measured where they are built.
    python tools/rk_bias_ab.py PARENT_LIB [reps] [out.txt] [U] [N]"""
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
L, K, d, Dc, topk, G = 200, 64, 768, 200, 100, 4
dt = torch.float16
g = torch.Generator(device=dev).manual_seed(5)
table = (torch.randn((N, d), generator=g, device=dev) / d ** 0.5).to(dt)
hid = torch.randint(0, N, (U, L), generator=g, device=dev, dtype=torch.int32)
mask = torch.ones((U, L), dtype=torch.bool, device=dev)
W1, Q, W2 = synthetic.init_weights(5, d, Dc, K, device=dev)
pk = corpus.pack_encoder(W1, Q, W2, dtype=dt)
mui, proj = corpus.encode_users(table, mask, pk, his_ids=hid)
sub = torch.sort(torch.randperm(N, generator=g, device=dev)[:N // 20]).values.to(torch.int32).contiguous()
torch.cuda.synchronize()

parent = ctypes.CDLL(parent_path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)   # its own symbols, not this build's
parent.miner_rank_topk.restype, parent.miner_rank_topk.argtypes = _lib.SIGNATURES["miner_rank_topk"]
parent.miner_abi_version.restype = ctypes.c_int
lib = _lib.lib()
assert parent.miner_abi_version() == _lib.ABI_VERSION and not hasattr(parent, "miner_rank_topk_biased"), \
    "PARENT_LIB is not the parent commit's library"
F16, W = _lib.DTYPE_F16, _lib.SCORE_WEIGHTED
stream = lambda: torch.cuda.current_stream().cuda_stream
ptr = lambda x: None if x is None else x.data_ptr()

# the prior at the spread of the scores (the unbiased top-k's scores say what that is)
s0 = torch.empty(U, topk, dtype=torch.float32, device=dev)
i0 = torch.empty(U, topk, dtype=torch.int32, device=dev)
assert lib.miner_rank_topk(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, topk, ptr(s0), ptr(i0)) == 0
scale = float(s0.std())
bias = (scale * torch.randn((G, N), generator=g, device=dev)).contiguous()
group = (torch.arange(U, device=dev) % G).to(torch.int32)


def rank(handle):
    s = torch.empty(U, topk, dtype=torch.float32, device=dev)
    i = torch.empty(U, topk, dtype=torch.int32, device=dev)
    rc = handle.miner_rank_topk(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, topk, ptr(s), ptr(i))
    assert rc == 0, rc
    return s, i


def rank_biased(b, grp, ids=None):
    s = torch.empty(U, topk, dtype=torch.float32, device=dev)
    i = torch.empty(U, topk, dtype=torch.int32, device=dev)

    def run():
        rc = lib.miner_rank_topk_biased(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, topk, None, 0, None,
                                        ptr(ids), -1 if ids is None else ids.numel(), ptr(s), ptr(i), None, 0,
                                        ptr(b), 0 if b is None else b.shape[0], ptr(grp))
        assert rc == 0, rc
        return s, i
    return run


def count(T, lists, b, grp):
    ts, ti = lists[0][:, :T].contiguous(), lists[1][:, :T].contiguous()
    out = torch.empty(U, T, dtype=torch.int32, device=dev)

    def run():
        rc = lib.miner_rank_count_biased(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, ptr(ts), ptr(ti), T,
                                         None, ptr(out), ptr(b), 0 if b is None else b.shape[0], ptr(grp))
        assert rc == 0, rc
        return (out,)
    return run


def pairs(ids, b, grp):
    C = ids.shape[1]
    out = torch.empty(U, C, dtype=torch.float32, device=dev)

    def run():
        rc = lib.miner_score_pairs_biased(stream(), F16, W, ptr(mui), ptr(proj), ptr(table), U, N, d, K, ptr(ids), C, ptr(out),
                                          ptr(b), 0 if b is None else b.shape[0], ptr(grp))
        assert rc == 0, rc
        return (out,)
    return run


b1 = bias[:1].contiguous()
plain = tuple(x.clone() for x in rank(lib))
l1 = tuple(x.clone() for x in rank_biased(b1, None)())
l4 = tuple(x.clone() for x in rank_biased(bias, group)())
torch.cuda.synchronize()

VARIANTS = {
    "a_parent_rank_topk": lambda: rank(parent), "b_rank_topk": lambda: rank(lib),
    "c_biased_G1": rank_biased(b1, None), "c_biased_G4": rank_biased(bias, group),
    "c_subset5": rank_biased(None, None, sub), "c_subset5_biased_G4": rank_biased(bias, group, sub),
    "d_count_T1": count(1, plain, None, None), "d_count_T1_biased_G4": count(1, l4, bias, group),
    "d_count_T64": count(64, plain, None, None), "d_count_T64_biased_G4": count(64, l4, bias, group),
    "e_pairs_C100": pairs(plain[1].contiguous(), None, None), "e_pairs_C100_biased_G4": pairs(l4[1].contiguous(), bias, group),
}


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


def add_check(lists, b, grp):
    """the listed scores are the unbiased pair scores plus the prior, one fp32 add (torch, on the device)"""
    ids = lists[1].contiguous()
    raw = pairs(ids, None, None)()[0]
    rows = torch.zeros(U, dtype=torch.long, device=dev) if grp is None else grp.long()
    want = raw + b[rows[:, None], ids.long().clamp(min=0)]
    return bool(torch.equal(want.view(torch.int32), lists[0].view(torch.int32)) and (ids >= 0).all())


same_ab = all(torch.equal(x, y) for x, y in zip(outs["a_parent_rank_topk"], outs["b_rank_topk"]))
exact = {"G1": add_check(outs["c_biased_G1"], b1, None), "G4": add_check(outs["c_biased_G4"], bias, group),
         "subset5 G4": add_check(outs["c_subset5_biased_G4"], bias, group)}
differs = bool((outs["c_biased_G4"][1] != outs["b_rank_topk"][1]).any(dim=1).all())
exact_d = {T: torch.equal(outs[f"d_count_T{T}_biased_G4"][0], torch.arange(T, dtype=torch.int32, device=dev).expand(U, T))
           for T in (1, 64)}
same_e = torch.equal(outs["e_pairs_C100_biased_G4"][0].view(torch.int32), l4[0].view(torch.int32))
med = {v: statistics.median(x) for v, x in ms.items()}
a, b_ = med["a_parent_rank_topk"], med["b_rank_topk"]
lines = [f"rk_bias_ab: U={U} N={N} L={L} K={K} d={d} fp16 weighted, {R} interleaved repeats, ms per call; "
         f"(a), (b): miner_rank_topk at topk={topk}; prior {scale:.4f} x randn [G={G}, N]"]
for v in VARIANTS:
    x = ms[v]
    lines.append(f"{v:24s} median {med[v]:8.3f}  min {min(x):8.3f}  max {max(x):8.3f}  "
                 f"spread {max(x) - min(x):6.3f}  all {[round(t, 3) for t in x]}")
diff = b_ - a
spread_a = max(ms["a_parent_rank_topk"]) - min(ms["a_parent_rank_topk"])
gate = abs(diff) <= spread_a
lines.append(f"(b) - (a) medians: {diff:+.3f} ms; (a)'s own spread {spread_a:.3f} ms -> "
             f"{'within' if gate else 'OUTSIDE'} it; (b) lists identical to (a): {same_ab}")
for v in ("c_biased_G1", "c_biased_G4"):
    lines.append(f"(c) {v}: {med[v]:8.3f} ms = {med[v] / b_:.3f} x (b)")
lines.append(f"(c) subset form, 5 % of the table ({sub.numel()} ids): unbiased {med['c_subset5']:8.3f} ms, biased G=4 "
             f"{med['c_subset5_biased_G4']:8.3f} ms = {med['c_subset5_biased_G4'] / med['c_subset5']:.3f} x it")
lines.append(f"(c) listed scores == unbiased pair scores + prior in torch fp32, bit for bit: {exact}; "
             f"every user's biased list differs from the unbiased one: {differs}")
for T in (1, 64):
    u_, bb = med[f"d_count_T{T}"], med[f"d_count_T{T}_biased_G4"]
    lines.append(f"(d) T={T:2d}: counting form unbiased {u_:8.3f} ms = {u_ / b_:.3f} x (b), biased G=4 {bb:8.3f} ms = "
                 f"{bb / u_:.3f} x the unbiased counting form; counts[u, j] == j: {exact_d[T]}")
u_, bb = med["e_pairs_C100"], med["e_pairs_C100_biased_G4"]
lines.append(f"(e) C={topk}: pair form unbiased {u_:8.3f} ms, biased G=4 {bb:8.3f} ms = {bb / u_:.3f} x it; "
             f"scores identical to the biased lists': {same_e}")
lines.append(f"library size: parent {os.path.getsize(parent_path)} bytes, this build {os.path.getsize(_lib.LIB_PATH)} bytes")
text = "\n".join(lines)
print(text, flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
sys.exit(0 if same_ab and all(exact.values()) and differs and all(exact_d.values()) and same_e else 1)
