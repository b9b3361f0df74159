#!/usr/bin/env python3
"""What an attention-knockout sweep costs: Pythia-2.8B-shaped synthetic weights
(fp16-valued: x2f16 with the exact-fp16 GEMMs), --prompts prompts of T = 15 tokens
(k-shot 4), one site per (prompt, window) for windows of --window layers, all
heads, the last token's attention to the demonstrations' label tokens blocked.

  (a) Model.patch_sweep_knockout against the SAME sites with the kind switched to
      SITE_REPLACE_HEADSET_LASTPOS and the same members (zero vectors): the
      planner gives both the same entry layers and rows, so the two sweeps differ
      by the knockout launches against the head-set patch launches.  Interleaved
      calls in one process on a filled trace; median and range of host clocks
      around work that ends in a device synchronise.  The knockout pass itself:
      HIP-event time and algorithmic bytes under TVR_HBM_ATTENTION of the profiled
      knockout sweep minus those of the profiled head-set sweep (same attention
      launches otherwise), and the achieved GB/s.
  (b) the PyTorch formulation on the same GPU: per window one batched fp32 forward
      of all prompts (the engine's processed weights) whose attention scores of
      the last query are masked_fill'ed in the window's layers.

The largest difference between (a)'s and (b)'s answer probabilities is reported.
Not a test and not part of bench.py.
  python tools/knockout_probe.py [--reps 10] [--prompts 52] [--window 8] [--model pythia-2.8b]"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tvr_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--prompts", type=int, default=52)
ap.add_argument("--kshot", type=int, default=4)
ap.add_argument("--window", type=int, default=8)
ap.add_argument("--model", default="pythia-2.8b")
a = ap.parse_args()
if a.reps < 1:
    ap.error("--reps must be positive")

model = tvr_amd.Model.from_pretrained(a.model, device="cuda", fp16_weights=True)
cfg = model.cfg
L, H, d, dh = cfg.n_layers, cfg.n_heads, cfg.d_model, cfg.d_head
KO, HS = tvr_amd._lib.SITE_ATTN_KNOCKOUT_LASTPOS, tvr_amd._lib.SITE_REPLACE_HEADSET_LASTPOS

seqs, answers = tvr_amd.prompts.synthetic_cie_prompts(model, a.prompts, a.kshot, seed=1234)
tg = np.asarray([int(x[0]) if isinstance(x, (list, tuple)) else int(x) for x in answers], dtype=np.int32)
n, T = len(seqs), len(seqs[0])
labels = [3 * (k + 1) for k in range(a.kshot)]  # BOS, then (x, f, y) per demonstration
windows = [(s, s + a.window - 1) for s in range(0, L - a.window + 1, a.window)]
W = len(windows)

sites = tvr_amd.make_sites(n * W)
sites["seq"] = np.repeat(np.arange(n, dtype=np.int32), W)
sites["kind"] = KO
sites["target"] = np.repeat(tg, W)
members = [np.asarray([(l, h, 0) for l in range(s, e + 1) for h in range(H)], dtype=np.int32) for s, e in windows]
off = np.concatenate([[0], np.cumsum(np.tile([len(m) for m in members], n))]).astype(np.int32)
pat = np.tile(np.concatenate(members), (n, 1))
koff = (np.arange(n * W + 1) * len(labels)).astype(np.int32)
keys = np.tile(np.asarray(labels, dtype=np.int32), n * W)
hs_sites = sites.copy()
hs_sites["kind"] = HS
zero = torch.zeros(1, d, device=model.device)

trace = model.trace(n, n * T)
model.forward_clean(seqs, trace=trace)


def knockout():
    return model.patch_sweep_knockout(trace, sites, off, pat, koff, keys)["prob"]


def headset():
    return model.patch_sweep_sets(trace, hs_sites, off, pat, zero)["prob"]


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


for _ in range(a.warmup):
    knockout(), headset()
tk, th = [], []
for _ in range(a.reps):  # interleaved: drift of the box hits both alike
    tk.append(clock(knockout))
    th.append(clock(headset))


def profiled(fn):
    model.profile(True)
    for _ in range(a.reps):
        fn()
    torch.cuda.synchronize()
    hb = model.profile_hbm_stats()["attention"]
    model.profile(False)
    return hb["ms"] / a.reps, hb["bytes"] / a.reps, hb["launches"] / a.reps


(ms_k, by_k, ln_k), (ms_h, by_h, ln_h) = profiled(knockout), profiled(headset)
ms, by = ms_k - ms_h, by_k - by_h

# ---- (b) PyTorch on the same GPU: the engine's processed fp32 weights, one masked forward per window
wts = model.weights
tok = torch.as_tensor(np.asarray(seqs, dtype=np.int64), device=model.device)
rd = cfg.rotary_dim
freq = cfg.rotary_base ** (torch.arange(rd // 2, device=model.device, dtype=torch.float32) / (rd / 2))
ang = torch.arange(T, device=model.device, dtype=torch.float32)[:, None] / torch.cat([freq, freq])[None, :]
cos, sin = torch.cos(ang)[None, :, None, :], torch.sin(ang)[None, :, None, :]
causal = torch.triu(torch.ones(T, T, dtype=torch.bool, device=model.device), diagonal=1)
tgd = torch.as_tensor(tg.astype(np.int64), device=model.device)


def ln(x):
    x = x - x.mean(-1, keepdim=True)
    return x / (x.pow(2).mean(-1, keepdim=True) + cfg.ln_eps).sqrt()


def rot(x):
    xr, xp = x[..., :rd], x[..., rd:]
    flip = torch.cat([-xr[..., rd // 2:], xr[..., :rd // 2]], -1)
    return torch.cat([xr * cos + flip * sin, xp], -1)


def torch_window(s, e):
    resid = wts.w_embed[tok]
    for l, lay in enumerate(wts.layers):
        y = ln(resid) @ lay.w1.T + lay.b1
        q, k, v = (y[..., i * d:(i + 1) * d].view(n, T, H, dh) for i in range(3))
        sc = torch.einsum("bqhe,bkhe->bhqk", rot(q), rot(k)) / math.sqrt(dh)
        sc = sc.masked_fill(causal, float("-inf"))
        if s <= l <= e:
            sc[:, :, -1, labels] = float("-inf")
        z = torch.einsum("bkhe,bhqk->bqhe", v, torch.softmax(sc, -1)).reshape(n, T, d)
        a2 = torch.cat([z, torch.nn.functional.gelu(y[..., 3 * d:])], -1)
        resid = resid + a2 @ lay.w2.T + lay.b2
    logits = ln(resid[:, -1]) @ wts.w_unembed_t.T + wts.b_unembed
    return torch.softmax(logits, -1).gather(1, tgd[:, None])[:, 0]


def baseline():
    return torch.stack([torch_window(s, e) for s, e in windows], 1).reshape(-1)


for _ in range(a.warmup):
    baseline()
tb = [clock(baseline) for _ in range(a.reps)]
pk, pb = knockout(), baseline()

out = {"model": a.model, "gemm": model.gemm, "exact16": model.exact16, "reps": a.reps, "prompts": n,
       "tokens_per_prompt": T, "windows": windows, "sites": n * W, "blocked_keys": labels,
       "knockout_sweep": stats(tk), "headset_sweep_same_sites": stats(th),
       "knockout_over_headset": round(statistics.median(tk) / statistics.median(th), 4),
       "knockout_pass": {"ms": round(ms, 5), "bytes": by, "launches": ln_k - ln_h,
                         "gbps": round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None},
       "pytorch": stats(tb), "knockout_over_pytorch": round(statistics.median(tk) / statistics.median(tb), 4),
       "max_prob_diff": float((pk - pb).abs().max()), "max_prob": float(pb.max())}
print(json.dumps(out))
