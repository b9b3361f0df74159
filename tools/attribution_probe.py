#!/usr/bin/env python3
"""What direct logit attribution from a trace costs next to the PyTorch formulation
a user would write today on the same GPU: Pythia-2.8B-shaped synthetic weights,
the bench's prompt shape (--prompts prompts of the k-shot length), a clean forward
into a trace, then

  engine    Model.logit_attribution(trace, targets, contrast): one direction pass,
            one head pass over every layer (csrc/logit_attribution.hpp)
  baseline  L + 1 Trace.resid_pre and L Trace.z reads, the final LayerNorm's scale,
            u = W_U[target] - W_U[contrast], then per layer (u / sigma) @ W_O and the
            z dot per head, and the centred residual dots

Times are host clocks around work that ends in a device synchronise (warm-up,
then --reps repetitions, the median reported).  The head pass's achieved GB/s is
its bytes (W_O as every chunk of 16 prompts reads it, the z and direction rows)
over its HIP-event time from tvr_profile_read_hbm (TVR_HBM_CAPTURE): the profiled
call with both outputs minus the profiled call with out_resid alone (the
direction pass).  The largest difference between the two results is reported
relative to the largest |value|.  Not a test and not part of bench.py.
  python tools/attribution_probe.py [--reps 20] [--prompts 12 96] [--kshot 4] [--model pythia-2.8b]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tvr_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--prompts", type=int, nargs="+", default=[12, 96])
ap.add_argument("--kshot", type=int, default=4)
ap.add_argument("--model", default="pythia-2.8b")
ap.add_argument("--weights", default="fp16", choices=["fp16", "fp32"],
                help="fp16-valued weights (the bench's default: exact-fp16 GEMMs) or fp32-valued")
a = ap.parse_args()
if a.reps < 1:
    ap.error("--reps must be positive")

model = tvr_amd.Model.from_pretrained(a.model, device="cuda", fp16_weights=a.weights == "fp16")
cfg = model.cfg
L, H, d = cfg.n_layers, cfg.n_heads, cfg.d_model
lib = model._lib


def timed(fn):
    for _ in range(a.warmup):
        fn()
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def probe(n_prompts):
    seqs, answers = tvr_amd.prompts.synthetic_cie_prompts(model, n_prompts, a.kshot, seed=1234)
    tg = [int(x[0]) if isinstance(x, (list, tuple)) else int(x) for x in answers]
    ct = [(t + 7) % cfg.d_vocab for t in tg]
    n = len(seqs)
    trace = model.trace(n, sum(map(len, seqs)))
    model.forward_clean(seqs, trace=trace)
    rows = torch.as_tensor([o + t - 1 for o, t in zip(trace.seq_offsets, trace.seq_lens)], device=model.device)
    tgd, ctd = torch.as_tensor(tg, device=model.device), torch.as_tensor(ct, device=model.device)
    WU = model.weights.w_unembed_t
    WO = [lay.w2[:, :d] for lay in model.weights.layers]

    def baseline():
        xL = trace.resid_pre(L)[rows]
        xc = xL - xL.mean(-1, keepdim=True)
        sigma = (xc.pow(2).mean(-1, keepdim=True) + cfg.ln_eps).sqrt()
        dirs = (WU[tgd] - WU[ctd]) / sigma
        resid, heads = [], []
        for l in range(L + 1):
            x = trace.resid_pre(l)[rows]
            resid.append(((x - x.mean(-1, keepdim=True)) * dirs).sum(-1))
        for l in range(L):
            g = dirs @ WO[l]
            heads.append((trace.z(l)[rows] * g).view(n, H, -1).sum(-1))
        return torch.stack(heads, 1), torch.stack(resid, 1)

    engine = lambda: model.logit_attribution(trace, tg, contrast=ct)  # noqa: E731
    res = {"prompts": n, "tokens_per_prompt": len(seqs[0]), "engine": timed(engine), "pytorch": timed(baseline)}
    res["engine_over_pytorch"] = round(res["engine"]["median_ms"] / res["pytorch"]["median_ms"], 4)
    (eh, er), (bh, br) = engine(), baseline()
    res["max_diff_heads_rel"] = float((eh - bh).abs().max() / bh.abs().max())
    res["max_diff_resid_rel"] = float((er - br).abs().max() / br.abs().max())

    # the head pass alone: HIP events, both outputs minus the direction pass
    heads = torch.empty(n, L, H, device=model.device)
    resid = torch.empty(n, L + 1, device=model.device)
    tga, cta = np.asarray(tg, dtype=np.int32), np.asarray(ct, dtype=np.int32)

    def profiled(out_head):
        model.profile(True)
        for _ in range(a.reps):
            tvr_amd._lib.check(lib.tvr_trace_logit_attribution(trace._h, None, tga.ctypes.data, cta.ctypes.data,
                                                               out_head, resid.data_ptr(), model._stream()), "probe")
        hb = model.profile_hbm_stats()["capture"]
        model.profile(False)
        return hb["ms"] / a.reps, hb["bytes"] / a.reps

    (ms_all, by_all), (ms_dir, by_dir) = profiled(heads.data_ptr()), profiled(None)
    ms, by = ms_all - ms_dir, by_all - by_dir
    res["direction_pass"] = {"ms": round(ms_dir, 5), "bytes": by_dir}
    res["head_pass"] = {"ms": round(ms, 5), "bytes": by, "gbps": round(by / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
                        "w_o_bytes_once": 4.0 * L * d * d}
    return res


out = {"model": a.model, "gemm": model.gemm, "exact16": model.exact16, "reps": a.reps,
       "runs": [probe(n) for n in a.prompts]}
print(json.dumps(out))
