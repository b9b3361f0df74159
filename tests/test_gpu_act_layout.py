"""GPU: the k-tile-interleaved x2f16 activation layout (split.hpp ACT_X2F16I, include/tvr.h TVR_ACT_X2F16_IL).

Logical [rows][K] as halves [rows][K / 32][2][32]: per row and 32-column group 64 B of plane 0, then 64 B of
plane 1 — one 128-B line, which the GEMM stages as whole lines (gemm_pingpong.hpp AIL).  Same values, same
fragments, same k order as the planar [rows][2][K] layout, so everything here is compared BITWISE:

* tvr_act_rows: the interleaved rows, de-interleaved on the host, are the planar planes; same range flag;
* tvr_gemm_planar on both layouts (two weight planes: the primitive ABI has no one-plane form), also against
  fp64 at the planar GEMM's bound;
* the engine on exact-fp16 weights, default layout against TVR_ACT_LAYOUT=planar: CIE sums (REPLACE_HEAD, fused
  sweep: the linearised entry on the 4-layer model), a head-set sweep, an ADD_ATTN_OUT_LASTPOS sweep and the
  trace's hook_z / hook_resid_pre.
"""
import numpy as np
import pytest
import torch

import tvr_amd

pytestmark = [pytest.mark.gpu]

X2F16 = tvr_amd._lib.GEMM_MODES["x2f16"]
X2F16_IL = 0x12  # include/tvr.h TVR_ACT_X2F16_IL


def _lib_stream():
    return tvr_amd._lib.load(), torch.cuda.current_stream().cuda_stream


def _deinterleave(il, K):
    """[rows][K / 32][2][32] halves -> [rows][2][K]."""
    rows = il.shape[0]
    return il.reshape(rows, K // 32, 2, 32).permute(0, 2, 1, 3).reshape(rows, 2, K)


def _act_rows(fmt, a, K, flag=None):
    lib, st = _lib_stream()
    rows, lda = a.shape
    out = torch.full((rows, 2 * K), -1, dtype=torch.int16, device="cuda")
    tvr_amd._lib.check(lib.tvr_act_rows(fmt, a.data_ptr(), lda, out.data_ptr(), rows, K,
                                        flag.data_ptr() if flag is not None else None, st), "act rows")
    return out


@pytest.mark.parametrize("rows,K", [(1, 32), (77, 96), (300, 2560)])
def test_act_rows_interleaved_is_planar_permuted(rows, K):
    g = torch.Generator().manual_seed(rows + K)
    a = torch.zeros(rows, K + 32)
    a[:, :K] = torch.randn(rows, K, generator=g) * 3
    a[:, K:] = 777.0  # the row padding is not read
    a = a.cuda()
    planar = _act_rows(X2F16, a, K).view(rows, 2, K)
    il = _act_rows(X2F16_IL, a, K)
    assert torch.equal(_deinterleave(il, K), planar)
    for big, want in ((4000.0, 0), (4100.0, 1)):
        a[rows // 2, K - 1] = big
        flags = []
        for fmt in (X2F16, X2F16_IL):
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            _act_rows(fmt, a, K, flag)
            flags.append(flag.item())
        assert flags == [want, want], (big, flags)
    lib, st = _lib_stream()
    out = torch.empty(rows, 2 * 48, dtype=torch.int16, device="cuda")
    assert lib.tvr_act_rows(X2F16_IL, a.data_ptr(), K + 32, out.data_ptr(), rows, 48, None, st) != 0  # K % 32


@pytest.mark.parametrize("M,N,K,pad", [(1, 1, 32, 0), (37, 130, 64, 0), (300, 257, 320, 0), (520, 512, 96, 32)])
def test_gemm_planar_interleaved_bitwise(M, N, K, pad):
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * 2e-2
    b = torch.randn(N, generator=g)
    lib, st = _lib_stream()
    Wd, bd = W.cuda(), b.cuda()
    scale = float(2.0 ** (15 - int(np.frexp(W.abs().max().item())[1])))
    planes = torch.empty(2, N, K, dtype=torch.int16, device="cuda")
    tvr_amd._lib.check(lib.tvr_weight_planes(X2F16, Wd.data_ptr(), scale, planes.data_ptr(), N * K, st), "split")
    lda = K + pad  # logical elements per row of the activation buffers (row stride 2 lda halves)
    Ap = torch.zeros(M, lda)
    Ap[:, :K] = A
    Ap = Ap.cuda()
    out = {}
    for fmt in (X2F16, X2F16_IL):
        Ah = _act_rows(fmt, Ap, lda)  # [M][2][lda] / [M][lda / 32][2][32]: the first K columns are A
        C = torch.full((M, N), float("nan"), device="cuda")
        tvr_amd._lib.check(lib.tvr_gemm_planar(fmt, Ah.data_ptr(), lda, planes.data_ptr(), K, N * K, scale,
                                               bd.data_ptr(), C.data_ptr(), N, M, N, K, st), "gemm")
        out[fmt] = C.cpu()
    ref = A.double() @ W.double().T + b.double()
    bound = 4e-7 * (A.double().abs() @ W.double().abs().T).max().item() + 1e-6
    for fmt, C in out.items():
        err = (C.double() - ref).abs().max().item()
        print(f"M {M} N {N} K {K} fmt {fmt:#x}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (fmt, err, bound)
    assert torch.equal(out[X2F16], out[X2F16_IL])


def _sites(rows, prompts):
    sites = tvr_amd.make_sites(len(rows))
    for s, row in zip(sites, rows):
        for k, v in row.items():
            s[k] = v
        s["target"] = prompts[row["seq"]][1]
    return sites


def _engine_results(cfg, sd, tok, layout, monkeypatch):
    if layout == "planar":
        monkeypatch.setenv("TVR_ACT_LAYOUT", "planar")
    else:
        monkeypatch.delenv("TVR_ACT_LAYOUT", raising=False)
    monkeypatch.setenv("TVR_LIN_ENTRY", "1")
    model = tvr_amd.Model.from_hf_state_dict(cfg, sd, device="cuda", tokenizer=tok, gemm="x2f16")
    assert model.exact16
    L, H, d = cfg.n_layers, cfg.n_heads, cfg.d_model
    g = torch.Generator().manual_seed(5)
    prompts = [[0] + torch.randint(1, cfg.d_vocab, (int(n),), generator=g).tolist() for n in (5, 9, 12, 7)]
    answers = [int(x) for x in torch.randint(0, cfg.d_vocab, (len(prompts),), generator=g)]
    mean = (torch.randn(L, H, d, generator=g) * 0.3).cuda()
    vecs = (torch.randn(L * H, d, generator=g) * 0.3).cuda()
    res = {"cie": tvr_amd.experiments.causal_indirect_effect_sums(mean, prompts, answers, model).clone()}
    trace = model.trace(len(prompts), sum(map(len, prompts)))
    model.forward_clean(prompts, trace=trace)
    for l in range(L):
        res[f"z{l}"] = trace.z(l).clone()
    for l in range(L + 1):
        res[f"resid_pre{l}"] = trace.resid_pre(l).clone()
    # head sets: two heads of one layer at all positions, heads of two layers at the last position
    set_rows = [dict(seq=i, kind=4 + i % 2) for i in range(len(prompts))]
    sets = [[(i % L, 0), (i % L, H - 1)] if i % 2 == 0 else [(0, 1), (L - 1, 2)] for i in range(len(prompts))]
    off, pat = [0], []
    for s in sets:
        pat += [(l, h, l * H + h) for l, h in s]
        off.append(len(pat))
    hs = model.patch_sweep_sets(trace, _sites(set_rows, prompts), np.asarray(off, np.int32),
                                np.asarray(pat, np.int32).reshape(-1, 3), vecs, topk=3, return_logits=True)
    add_rows = [dict(seq=i, kind=2, layer=l, vec=(i + l) % (L * H)) for i in range(len(prompts)) for l in range(L)]
    add = model.patch_sweep(trace, _sites(add_rows, prompts), vecs, topk=3, return_logits=True)
    for name, o in (("headset", hs), ("add_attn_out", add)):
        for k in ("logits", "prob", "topk"):
            res[f"{name}_{k}"] = o[k].clone()
    del trace, model
    torch.cuda.empty_cache()
    return res


@pytest.mark.parametrize("n_layers", [2, 4])  # 2: tests/test_gpu_exact16.py's tiny model; 4: with a linearised entry layer
def test_engine_layouts_bitwise(n_layers, tokenizer, monkeypatch):
    cfg = tvr_amd.get_config("tiny")
    if n_layers != cfg.n_layers:
        cfg = cfg.with_(n_layers=n_layers)
    sd = tvr_amd.weights.synth_hf_state_dict(cfg, seed=0, std=0.3, fp16=True)
    a = _engine_results(cfg, sd, tokenizer, "interleaved", monkeypatch)
    b = _engine_results(cfg, sd, tokenizer, "planar", monkeypatch)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.isfinite(a[k].double()).all(), k
        assert torch.equal(a[k], b[k]), (k, (a[k].double() - b[k].double()).abs().max().item())
    assert a["cie"].abs().max().item() > 0
