#!/usr/bin/env python3
"""What per-source-token logit attribution from a trace costs next to the PyTorch
formulation a user would write today on the same GPU: Pythia-2.8B-shaped synthetic
weights, the bench's prompt shape (--prompts prompts of the k-shot length), a clean
forward into a trace, then, interleaved in this one process,

  engine    Model.source_attribution(trace, targets, contrast, want_keys=True): the
            direction pass, then per group of layers the G pass and the source
            kernel (csrc/source_attribution.hpp)
  pattern   Model.capture_pattern(trace, want_pattern=True) alone: the kernel the
            source kernel extends (its bytes: the Q row + the K rows)
  baseline  Trace.attention_pattern, the final LayerNorm's scale and
            u = W_U[target] - W_U[contrast], then per layer Trace.v, (u / sigma) @ W_O
            and an einsum of the pattern, V and g per head

Times are host clocks around work that ends in a device synchronise (warm-up,
then --reps repetitions; median and range reported).  The two spans of the engine
call are its HIP-event times from tvr_profile_read_hbm: TVR_HBM_CAPTURE (the
direction and G passes) and TVR_HBM_ATTENTION (the source kernel), each with the
bytes its kernels request and the rate they give; the pattern call's span likewise.
At these sizes the trace's rows sit in the Infinity Cache: the rates are not HBM
figures.  The largest difference between the two results is reported relative to
the largest |value|.  Not a test and not part of bench.py.
  python tools/source_probe.py [--reps 20] [--prompts 12 96] [--kshot 4] [--model pythia-2.8b]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
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


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def timed_interleaved(fns):
    """Every function once per round, in turn (the same process, the same clocks): {name: summary}."""
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t) * 1e3)
    return {k: summary(v) for k, v in ts.items()}


def probe(n_prompts):
    seqs, answers = tvr_amd.prompts.synthetic_cie_prompts(model, n_prompts, a.kshot, seed=1234)
    tg = [int(x[0]) if isinstance(x, (list, tuple)) else int(x) for x in answers]
    ct = [(t + 7) % cfg.d_vocab for t in tg]
    n = len(seqs)
    trace = model.trace(n, sum(map(len, seqs)))
    model.forward_clean(seqs, trace=trace)
    lens = trace.seq_lens
    T = max(lens)
    rows = torch.as_tensor([o + t - 1 for o, t in zip(trace.seq_offsets, lens)], device=model.device)
    # token index of key j of sequence s (clamped: the pattern is zero beyond a sequence's length)
    idx = torch.as_tensor([[o + min(j, t - 1) for j in range(T)] for o, t in zip(trace.seq_offsets, lens)],
                          device=model.device)
    tgd, ctd = torch.as_tensor(tg, device=model.device), torch.as_tensor(ct, device=model.device)
    WU = model.weights.w_unembed_t
    WO = [lay.w2[:, :d] for lay in model.weights.layers]

    def baseline():
        pat = trace.attention_pattern()                      # [n, L, H, T]
        xL = trace.resid_pre(L)[rows]
        xc = xL - xL.mean(-1, keepdim=True)
        sigma = (xc.pow(2).mean(-1, keepdim=True) + cfg.ln_eps).sqrt()
        dirs = (WU[tgd] - WU[ctd]) / sigma
        out = []
        for l in range(L):
            g = (dirs @ WO[l]).view(n, H, -1)
            v = trace.v(l)[idx].view(n, T, H, -1)
            out.append(pat[:, l] * torch.einsum("sjhe,she->shj", v, g))
        return torch.stack(out, 1)

    engine = lambda: model.source_attribution(trace, tg, contrast=ct, want_keys=True)[0]  # noqa: E731
    pattern = lambda: model.capture_pattern(trace, want_pattern=True)[0]  # noqa: E731
    res = {"prompts": n, "tokens_per_prompt": len(seqs[0])}
    res.update(timed_interleaved({"engine": engine, "pattern": pattern, "pytorch": baseline}))
    res["engine_over_pytorch"] = round(res["engine"]["median_ms"] / res["pytorch"]["median_ms"], 4)
    e, b = engine(), baseline()
    res["max_diff_rel"] = float((e - b).abs().max() / b.abs().max())

    def spans(fn):
        model.profile(True)
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        hb = model.profile_hbm_stats()
        model.profile(False)
        return {k: {"ms": round(hb[k]["ms"] / a.reps, 5), "bytes": hb[k]["bytes"] / a.reps,
                    "gbps": round(hb[k]["bytes"] / (hb[k]["ms"] * 1e-3) / 1e9, 1) if hb[k]["ms"] > 0 else None}
                for k in ("capture", "attention")}

    sp, pp = spans(engine), spans(pattern)
    res["engine_spans"] = {"direction_and_g_pass": sp["capture"], "source_kernel": sp["attention"]}
    res["pattern_span"] = pp["attention"]
    res["source_over_pattern_bytes"] = round(sp["attention"]["bytes"] / pp["attention"]["bytes"], 3)
    res["source_over_pattern_ms"] = round(sp["attention"]["ms"] / pp["attention"]["ms"], 3) if pp["attention"]["ms"] else None
    return res


out = {"model": a.model, "gemm": model.gemm, "exact16": model.exact16, "reps": a.reps, "warmup": a.warmup,
       "runs": [probe(n) for n in a.prompts]}
print(json.dumps(out))
