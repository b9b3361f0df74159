"""The one-plane GEMM at the probe's two shapes with the engine's launch arguments, plain weight plane against the
row-pair-interleaved one (tvr_gemm_launch exact16 = 1 / 2), alternately in one process.

tools/gemm_split_probe times the kernel with the plain bias epilogue.  The engine launches it with the residual
epilogue in place (O + MLP-out), with the GELU epilogue and a second A operand from column 3d (QKV + MLP-in) and
with gathered rows; this tool times those forms, so a gain that differs between the probe and the bench can be
placed.  One JSON line per (shape, form): ms of every run of each layout and the ratio of the medians.
  python3 tools/w_layout_probe.py [--rounds 3] [--m 90000]
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import tvr_amd  # noqa: E402

L = tvr_amd._lib
IL = 0x12
BIAS, GELU, RESID = 0, 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--m", type=int, default=90000)
    a = ap.parse_args()
    cfg = tvr_amd.config.PythiaConfig(1, 64, 4, 32, 64, n_ctx=32, name="w-layout-probe")
    model = tvr_amd.Model(cfg, tvr_amd.weights.synth_engine_weights(cfg, seed=1, device="cuda"),
                          tokenizer=tvr_amd.tokenizer.SyntheticTokenizer(512), device="cuda", gemm="f32")
    lib, h, M = model._lib, model._h, a.m
    g = torch.Generator(device="cuda").manual_seed(1)
    for shape, N, K, forms in (("qkv_mlpin", 17920, 2560, ("bias", "gelu", "gelu+a2", "gelu+a2+rows")),
                               ("o_mlpout", 2560, 12800, ("bias", "resid", "resid+rows"))):
        A = torch.randn(M, 2 * K, generator=g, device="cuda").half().view(torch.int16)  # both planes: N(0, 1) values
        A2 = torch.randn(M, 2 * K, generator=g, device="cuda").half().view(torch.int16)
        W1 = (torch.randn(N, K, generator=g, device="cuda") * 0.02).half().view(torch.int16)
        W2 = torch.empty_like(W1)
        L.check(lib.tvr_weight_rows_il(W1.data_ptr(), W2.data_ptr(), N, K, model._stream()), "tvr_weight_rows_il")
        bias = torch.randn(N, device="cuda")
        n_split = 7680 if shape == "qkv_mlpin" else 0
        out0 = torch.empty(M, N, device="cuda")
        out1h = torch.empty(M, 2 * (N - n_split), dtype=torch.int16, device="cuda") if n_split else None
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        perm = torch.randperm(M).tolist()
        rows = (ctypes.c_int32 * M)(*perm)
        for form in forms:
            epi = GELU if form.startswith("gelu") else RESID if form.startswith("resid") else BIAS
            args = L.CGemmArgs(fmt=IL, exact16=1, epi=epi, form=L.FORM_PLAN, slicing=L.SLICE_MODEL, M=M, N=N, K=K, lda=K,
                               ldw=K, ld0=N, w_scale=1.0, wps=0, A=A.data_ptr(), bias=bias.data_ptr(),
                               out0=out0.data_ptr())
            if epi == GELU:
                args.n_split, args.out1h, args.ld1h, args.ps1h = n_split, out1h.data_ptr(), 2 * (N - n_split), 0
                args.range_flag = flag.data_ptr()
            if epi == RESID:  # in place, as run_block_out
                args.resid, args.ldr = out0.data_ptr(), N
            if "a2" in form:
                args.a2, args.a2_col = A2.data_ptr(), n_split
            if "rows" in form:
                args.a_rows = args.out_rows = ctypes.cast(rows, ctypes.c_void_p)
                args.a_buf_rows = args.out_buf_rows = M
            ms = {1: [], 2: []}
            for r in range(a.rounds + 1):  # round 0: warm-up
                for x16, W in ((1, W1), (2, W2)):
                    args.exact16, args.W = x16, W.data_ptr()
                    if epi == RESID:
                        out0.zero_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    L.check(lib.tvr_gemm_launch(h, ctypes.byref(args), model._stream()), "tvr_gemm_launch")
                    e1.record()
                    e1.synchronize()
                    if r:
                        ms[x16].append(round(e0.elapsed_time(e1), 3))
            med = {k: statistics.median(v) for k, v in ms.items()}
            print(json.dumps({"shape": shape, "form": form, "M": M, "N": N, "K": K, "ms_rows": ms[1], "ms_il": ms[2],
                              "tflops_rows": round(2e-9 * M * N * K / med[1], 1),
                              "tflops_il": round(2e-9 * M * N * K / med[2], 1),
                              "gain": round(med[1] / med[2] - 1.0, 4),
                              "timing": "events around tvr_gemm_launch (with rows: its index upload included)"}),
                  flush=True)
        del A, A2, W1, W2, out0, out1h
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
