#!/usr/bin/env python3
"""Measure the residual-stream task-vector path at the C2 shape on one GPU
(seeded synthetic Pythia-2.8B; DESIGN.md section 3.5 records one run):

  python tools/task_vector_probe.py [--gemm x2f16] [--fp16-weights] [--reps 5] > profiles/task_vectors.json

* sweeps: ``apply_task_vectors_to_zero_shot`` (kind-6 sites, entry at layer l)
  beside ``apply_layered_vectors_to_zero_shot`` (kind-2 sites, entry at layer
  l + 1) on the same 52 zero-shot prompts x 32 layers, alternating, each call
  timed by a host clock around a device synchronise; sites/s from the median.
* capture: ``extract_task_vectors`` at N = 2048, 6-shot with separators (T = 28): the whole
  call's prompts/s, and the capture kernels' GB/s from ``profile_hbm_stats``
  (HIP events around the launch pair, algorithmic bytes) in a pass of its own.
"""
import argparse
import json
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import tvr_amd  # noqa: E402
from tvr_amd import experiments as E  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="pythia-2.8b")
    ap.add_argument("--gemm", default="x2f16")
    ap.add_argument("--fp16-weights", action="store_true", help="fp16-valued weights: the exact-fp16 GEMMs "
                    "(the trace is then uncentred and the capture centres each row)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--contexts", type=int, default=2048)
    args = ap.parse_args()
    model = tvr_amd.Model.from_pretrained(args.model, device="cuda", gemm=args.gemm, fp16_weights=args.fp16_weights)
    task, arrow = tvr_amd.tasks.letter_to_caps, tvr_amd.tasks.ARROW
    L = model.cfg.n_layers
    random.seed(0)  # warm at the timed size: the scratch trace is allocated here
    E.extract_task_vectors(task, arrow, model, num_contexts=args.contexts, len_contexts=6, seperator_token=",")
    random.seed(1)
    theta, t_ex = timed(lambda: E.extract_task_vectors(task, arrow, model, num_contexts=args.contexts, len_contexts=6, seperator_token=","))
    # the capture alone, profiled in its own pass (events around the launch pair)
    random.seed(1)
    prompts = tvr_amd.prompts.sample_icl_prompts(model, task, arrow, ",", args.contexts, 6)
    trace = model._sweep_trace(len(prompts), sum(map(len, prompts)))  # the extraction's own (one trace this size)
    model.forward_clean(prompts, trace=trace)
    model.capture_resid(trace)  # warm
    model.profile(True)
    for _ in range(args.reps):
        model.capture_resid(trace)
    torch.cuda.synchronize()
    cap = model.profile_hbm_stats()["capture"]
    model.profile(False)
    del trace
    random.seed(2)
    mean = E.generate_mean_activation(task, arrow, model=model, num_contexts=64, len_contexts=6)
    lv = E.gather_head_activations_to_layers(mean)
    sweeps = {"task_vectors": lambda: E.apply_task_vectors_to_zero_shot(theta, task, arrow, model),
              "layered_vectors": lambda: E.apply_layered_vectors_to_zero_shot(lv, task, arrow, model)}
    times = {k: [] for k in sweeps}
    for k, fn in sweeps.items():
        fn()  # warm
    for _ in range(args.reps):  # alternating
        for k, fn in sweeps.items():
            times[k].append(timed(fn)[1])
    n_sites = len(task) * L
    res = {"model": args.model, "gemm": model.gemm, "exact16": model.exact16, "device": torch.cuda.get_device_name(0),
           "sites": n_sites, "reps": args.reps,
           "sweep_sites_per_s": {k: round(n_sites / statistics.median(v), 1) for k, v in times.items()},
           "sweep_s": {k: [round(x, 5) for x in v] for k, v in times.items()},
           "extraction": {"prompts": args.contexts, "tokens_per_prompt": len(prompts[0]), "s": round(t_ex, 4),
                          "prompts_per_s": round(args.contexts / t_ex, 1)},
           "capture": {"launches": cap["launches"], "ms_per_call": round(cap["ms"] / max(cap["launches"], 1), 4),
                       "bytes_per_call": cap["bytes"] / max(cap["launches"], 1),
                       "gbps": round(cap["gbps"], 1) if cap["gbps"] else None}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
