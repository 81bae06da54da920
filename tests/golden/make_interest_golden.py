"""Generate tests/golden/interest/corpus_interest_*.npz: which of a user's K interests the REFERENCE's own Miner
(src/model/model.py) matched each news with, for the c5_weighted and c5_max cases of
make_corpus_golden.py (the same seeds, so the same model, table and histories: the recorded scores
must equal corpus_<case>.npz's, which is what identifies the case).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_interest_golden.py

Recorded per case, [U, N] each, from the reference's own forward pass and nothing else:
  scores    the click scores (float32), as in corpus_<case>.npz
  interest  'weighted': the arg-max over K of the target-aware softmax weights (model.py:213), seen
            by wrapping the functional softmax that model.py calls; 'max': the index that
            Tensor.max(dim=2) (model.py:129) returns                                    (int32)
  margin    'weighted': log(w1 / w2) of the two largest weights; 'max': the gap of the two largest
            M_k                                                                         (float32)
Data only: no reference code is stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np

REF = os.environ.get("MINER_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    if not os.path.isdir(os.path.join(REF, "src")):
        print(f"reference not found at {REF}: skipping")
        return 0
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import torch
    import torch.nn as nn
    import src.model.model as ref_model                    # noqa: E402  (reference)

    class StubNewsEncoder(nn.Module):
        def __init__(self, table):
            super().__init__()
            self.embed_dim = table.shape[1]
            self.register_buffer("table", table)

        def forward(self, title_encoding, title_attn_mask, sapo_encoding=None, sapo_attn_mask=None):
            return self.table[title_encoding[:, 0]]

    def run_case(name, *, U, L, K, Dc, d, N, score_type, seed, hist_len):
        rng = np.random.default_rng(seed)
        table = (rng.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)   # row 0 = the pad news
        his_ids = np.zeros((U, L), np.int64)
        for u in range(U):
            n = int(hist_len[u])
            his_ids[u, L - n:] = rng.integers(1, N, size=n)                     # left-padded (reader.py:369)
        his_mask = his_ids != 0
        torch.manual_seed(seed)
        model = ref_model.Miner(StubNewsEncoder(torch.from_numpy(table)), False, K, Dc, score_type, 0.2).eval()
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
        cand = np.tile(np.arange(N), (U, 1))                                    # every news is a candidate
        seen = {}
        real_softmax, real_max = ref_model.torch_f.softmax, torch.Tensor.max

        def softmax(x, *a, **kw):
            w = real_softmax(x, *a, **kw)
            if tuple(w.shape) == (U, N, K):                 # the target-aware weights (poly attention: [U, K, L])
                seen["weights"] = w.detach().clone()
            return w

        def tmax(self, *a, **kw):
            r = real_max(self, *a, **kw)
            if tuple(self.shape) == (U, N, K) and (kw.get("dim") == 2 or (a and a[0] == 2)):
                seen["m"], seen["index"] = self.detach().clone(), r[1].detach().clone()
            return r

        ref_model.torch_f.softmax, torch.Tensor.max = softmax, tmax
        try:
            with torch.no_grad():
                title, his = t(cand)[..., None], t(his_ids)[..., None]
                ones = lambda x: torch.ones_like(x, dtype=torch.bool)
                mui, scores = model(title=title, title_mask=ones(title), his_title=his, his_title_mask=ones(his),
                                    his_mask=t(his_mask), sapo=title, sapo_mask=ones(title), his_sapo=his,
                                    his_sapo_mask=ones(his))
        finally:
            ref_model.torch_f.softmax, torch.Tensor.max = real_softmax, real_max
        if score_type == "weighted":
            w = seen["weights"]
            interest = w.argmax(dim=2)
            top2 = torch.topk(w, 2, dim=2).values
            margin = torch.log(top2[..., 0] / top2[..., 1])
        else:
            interest = seen["index"]
            top2 = torch.topk(seen["m"], 2, dim=2).values
            margin = top2[..., 0] - top2[..., 1]
        old = np.load(os.path.join(OUT, f"corpus_{name}.npz"), allow_pickle=False)
        assert np.array_equal(old["scores"], scores.numpy()), f"{name}: not the case corpus_{name}.npz holds"
        os.makedirs(os.path.join(OUT, "interest"), exist_ok=True)   # a folder of their own: tests glob golden/corpus_*.npz
        path = os.path.join(OUT, "interest", f"corpus_interest_{name}.npz")
        np.savez_compressed(path, scores=scores.numpy(), interest=interest.numpy().astype(np.int32),
                            margin=margin.numpy().astype(np.float32))
        print(f"{name}: interest [{U}, {N}] -> {os.path.getsize(path) / 1e3:.1f} KB; per user the share of its "
              f"most frequent interest {[round(float(np.bincount(r, minlength=K).max()) / N, 3) for r in interest.numpy()]}")

    # the two cases of make_corpus_golden.py that have a dominant interest, argument for argument
    run_case("c5_weighted", U=5, L=200, K=64, Dc=200, d=128, N=700, score_type="weighted", seed=51,
             hist_len=[200, 37, 0, 150, 1])
    run_case("c5_max", U=3, L=200, K=64, Dc=200, d=128, N=600, score_type="max", seed=52, hist_len=[200, 90, 3])
    return 0


if __name__ == "__main__":
    sys.exit(main())
