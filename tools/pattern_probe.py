#!/usr/bin/env python3
"""What the attention-pattern capture costs next to the clean forward that pays
for its data: Pythia-2.8B-shaped synthetic weights, the headline sweep's prompt
shape (32 prompts, the bench's k-shot), a clean forward into a trace and
tvr_trace_capture_pattern on that trace with and without the per-role mass.

Times are host clocks around work that ends in a device synchronise (warm-up,
then --reps repetitions, the median reported); the capture's achieved GB/s is
its algorithmic bytes over its HIP-event time from tvr_profile_read_hbm
(TVR_HBM_ATTENTION), taken in a separate profiled pass.  Not a test and not part
of bench.py.
  python tools/pattern_probe.py [--reps 20] [--prompts 32] [--kshot 4] [--model pythia-2.8b]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import tvr_amd  # noqa: E402
from tvr_amd.prompts import ROLES  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--prompts", type=int, default=32)
ap.add_argument("--kshot", type=int, default=4)
ap.add_argument("--model", default="pythia-2.8b")
ap.add_argument("--weights", default="fp16", choices=["fp16", "fp32"],
                help="fp16-valued weights (the bench's default: exact-fp16 GEMMs) or fp32-valued")
a = ap.parse_args()
if a.reps < 1:
    ap.error("--reps must be positive")

model = tvr_amd.Model.from_pretrained(a.model, device="cuda", fp16_weights=a.weights == "fp16")
seqs, _ = tvr_amd.prompts.synthetic_cie_prompts(model, a.prompts, a.kshot, seed=1234)
T = len(seqs[0])
# BOS, k demos of (input, function, label), the query and its function token: prompts.ROLES by position
roles = [[0] + [1, 2, 3] * a.kshot + [5, 6] for _ in seqs]
assert all(len(r) == len(s) for r, s in zip(roles, seqs))
trace = model.trace(len(seqs), sum(map(len, seqs)))


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
    return ts


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


forward = timed(lambda: model.forward_clean(seqs, trace=trace))
pattern = timed(lambda: trace.attention_pattern())
mass = timed(lambda: trace.attention_mass(roles, len(ROLES)))
both = timed(lambda: model.capture_pattern(trace, classes=roles, n_classes=len(ROLES), want_pattern=True))

res = {"model": a.model, "gemm": model.gemm, "exact16": model.exact16, "prompts": len(seqs), "tokens_per_prompt": T,
       "reps": a.reps, "clean_forward": summary(forward), "capture_pattern": summary(pattern),
       "capture_mass": summary(mass), "capture_pattern_and_mass": summary(both)}
fwd = res["clean_forward"]["median_ms"]
for k in ("capture_pattern", "capture_mass", "capture_pattern_and_mass"):
    res[k]["share_of_clean_forward"] = round(res[k]["median_ms"] / fwd, 5)

# the kernel alone: HIP events around the launch, algorithmic bytes (Q row + K rows read, outputs written)
for name, fn in (("capture_pattern", lambda: trace.attention_pattern()),
                 ("capture_mass", lambda: trace.attention_mass(roles, len(ROLES))),
                 ("capture_pattern_and_mass", lambda: model.capture_pattern(trace, classes=roles, n_classes=len(ROLES),
                                                                            want_pattern=True))):
    model.profile(True)
    for _ in range(a.reps):
        fn()
    hb = model.profile_hbm_stats()["attention"]
    model.profile(False)
    res[name]["kernel"] = {"launches": hb["launches"], "ms_per_launch": round(hb["ms"] / max(hb["launches"], 1), 5),
                           "bytes_per_launch": hb["bytes"] / max(hb["launches"], 1),
                           "gbps": round(hb["gbps"], 1) if hb["gbps"] else None}
print(json.dumps(res))
