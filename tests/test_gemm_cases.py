"""CPU: the planar-GEMM cases of tests/gemm_cases.py are what they claim to be.

The fp64 reference against torch's fp64 matmul of the decoded planes; the
integer cases stay below 2^24 in every partial sum and their planes are exact;
the one-hot cases select a decoded weight exactly; both fp32 restatements sit
inside the bar they set, on graded shapes of every family the GPU file runs
(it computes each case's bar with the same code); the GELU
restatement against torch.nn.functional.gelu in fp64; the layouts round-trip;
the raster covers every tile once.  Then the ABI of ``tvr_gemm_launch``: the
symbol, the struct against the header, and every refusal (no device is touched:
the arguments are checked before the model is read).
"""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import gemm_cases as G
import tvr_amd

L = tvr_amd._lib
ROOT = Path(__file__).resolve().parents[1]

# (fmt, M, N, K, one_plane): graded shapes of tests/test_gpu_gemm_forms.py, every family and K range
GRADED = [(G.X2F16, 300, 260, 512, False), (G.X2F16, 300, 260, 768, True), (G.X2F16, 300, 260, 4096, False),
          (G.X2F16, 300, 260, 544, True), (G.X2F16, 300, 260, 2080, False), (G.BF16, 300, 260, 1024, False),
          (G.BF16, 300, 260, 1088, False), (G.X2F16, 17, 130, 96, False), (G.X2F16, 1, 256, 16384, False),
          (G.X2F16, 1, 256, 16384, True), (G.X2F16, 16, 260, 160, False), (G.BF16, 15, 260, 192, False)]


@pytest.mark.parametrize("fmt,M,N,K,one", GRADED[:6] + GRADED[7:9])
def test_reference_is_the_fp64_matmul_of_the_decoded_planes(fmt, M, N, K, one):
    c = G.Case("graded", fmt, M, N, K, one_plane=one, seed=3)
    want = torch.from_numpy(c.Ad) @ torch.from_numpy(c.Wd).T
    assert np.abs(c.ref - want.numpy()).max() <= 1e-13 * c.denom().max()
    # the decoded planes are the operands to 2^-22 (x2f16) / 2^-9 (bf16), apart from fp16's subnormal spacing
    rel = 2.0 ** -8 if fmt == G.BF16 else 2.0 ** -21
    assert (np.abs(c.Ad - c.A) <= rel * np.abs(c.A) + 2.0 ** -25 / 16).all()
    assert (np.abs(c.Wd - c.W) <= rel * np.abs(c.W) + 2.0 ** -25 / c.wscale).all()
    assert np.abs(c.A).max() < 4095.0  # inside the x2f16 split's range


@pytest.mark.parametrize("fmt", [G.X2F16, G.BF16])
def test_integer_cases_are_exact_and_below_2_to_24(fmt):
    for M, N, K in ((300, 260, 4096), (513, 516, 192), (1, 256, 16384), (17, 130, 64)):
        assert G.int_bound(K) < 2 ** 24
        c = G.Case("int", fmt, M, N, K)
        assert np.abs(c.A).max() <= 6 and np.abs(c.W).max() <= 8
        assert np.abs(c.bias).max() <= 11 and np.abs(c.resid).max() <= 14
        # every row, column and k position has its own operand pattern: a swapped tile or slice changes a result
        assert len({r.tobytes() for r in c.A[:13]}) == min(M, 13) and len({r.tobytes() for r in c.W[:17]}) == 17
        # the worst partial sum in any order: sum of |products|
        assert (np.abs(c.A.astype(np.float64)) @ np.abs(c.W.astype(np.float64)).T).max() + 25 <= G.int_bound(K)
        # exact planes: plane 0 holds the value, the residual planes are zero, the scales are powers of two
        assert np.array_equal(c.Ad, c.A.astype(np.float64)) and np.array_equal(c.Wd, c.W.astype(np.float64))
        if fmt == G.X2F16:
            assert not G.plane_values(c.ap, fmt)[1].any() and not G.plane_values(c.wp, fmt)[1].any()
            assert np.log2(c.wscale) % 1 == 0 and np.abs(G.plane_values(c.wp, fmt)[0]).max() <= 65504
        want = c.A.astype(np.int64) @ c.W.astype(np.int64).T
        assert np.array_equal(c.ref, want.astype(np.float64))
        for epi in (G.EPI_BIAS, G.EPI_RESID):
            e = c.expect(epi)
            assert np.array_equal(e, np.round(e)) and np.abs(e).max() < 2 ** 24
            for order in ("serial", "pairwise"):  # and the fp32 restatements return it bit for bit
                assert np.array_equal(G.restate(c, order, epi).astype(np.float64), e)
                assert np.array_equal(G.restate(c, order, epi, two_products=True).astype(np.float64), e)


@pytest.mark.parametrize("fmt,one", [(G.X2F16, False), (G.X2F16, True), (G.BF16, False)])
def test_onehot_cases_select_a_decoded_weight(fmt, one):
    M, N, K = 300, 260, 192
    c = G.Case("onehot", fmt, M, N, K, one_plane=one)
    k = G.onehot_k(M, K)
    assert set(k % 64) == set(range(64)) and set(k // 32) == set(range(K // 32))  # every position, every k-tile
    want = c.Wd[:, k].T
    assert np.array_equal(c.ref, want)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)  # the plane sum fits fp32
    for order in ("serial", "pairwise"):
        assert np.array_equal(G.restate(c, order, two_products=one).astype(np.float64), want)


@pytest.mark.parametrize("fmt,M,N,K,one", GRADED)
def test_both_restatements_sit_inside_the_bar(fmt, M, N, K, one):
    c = G.Case("graded", fmt, M, N, K, one_plane=one, seed=3)
    for epi in (G.EPI_BIAS, G.EPI_RESID):
        bar, e_serial, e_pair = c.bar(epi, two_products=one)
        want = c.expect(epi)
        for order in ("serial", "pairwise"):
            got = G.restate(c, order, epi, one).astype(np.float64)
            assert (np.abs(got - want) <= bar).all()
        assert (bar >= np.spacing(np.abs(want).astype(np.float32))).all()  # never below the store's own rounding
        # the bar is a statement about fp32 arithmetic: far below the project's 1e-4, far above fp64 noise
        assert 1e-9 < max(e_serial, e_pair) < (2e-3 if fmt == G.BF16 else 1e-5)
    # the magnitudes really spread over decades, and the residual planes matter
    col = np.abs(c.A).max(axis=0)
    assert col.max() / col.min() > 1e4
    if fmt == G.X2F16 and not one:
        assert G.plane_values(c.wp, fmt)[1].any() and np.abs(c.W).max() < 1e-2


def test_gelu_restatement_against_torch_fp64():
    x = np.concatenate([np.linspace(-12, 12, 200001), [4000.0, 4100.0, -4100.0, 0.0, -0.0, 1e-30, -1e-30],
                        np.random.default_rng(0).standard_normal(20000) * 50]).astype(np.float32)
    want = torch.nn.functional.gelu(torch.from_numpy(x).double()).numpy()
    assert np.array_equal(G.gelu64(x), want)
    err = np.abs(G.gelu_restate(x).astype(np.float64) - want) / np.maximum(1.0, np.abs(x))
    assert err.max() < 2.5e-7  # csrc/gemm_f32.hpp: |error| <= 1.7e-7 max(1, |x|) (A&S 7.1.26 + fp32 rounding)
    for fmt in (G.X2F16, G.BF16):
        bar, e = G.gelu_bar(x, fmt)
        assert e == err.max() and (bar >= 4 * e).all() and bar.max() < 4100 * (2e-6 if fmt == G.X2F16 else 5e-3)
    # exact landmarks: the range-flag cases' values pass through unchanged
    assert G.gelu_restate(np.float32([4100.0, 4000.0, -4100.0])).tolist() == [4100.0, 4000.0, 0.0]


def test_layouts_round_trip_and_poison():
    rng = np.random.default_rng(1)
    planes = rng.integers(0, 0x7C00, size=(2, 5, 64), dtype=np.uint16)
    for fmt in (G.X2F16, G.IL, G.BF16):
        buf = G.act_buffer(planes, fmt, ld=96, rows_total=7)
        log = G.act_logical(buf, fmt, 96)
        assert np.array_equal(log[:, :5, :64], planes)
        assert (log[:, :5, 64:] == G.NAN16[fmt]).all() and (log[:, 5:] == G.NAN16[fmt]).all()
    il = G.act_buffer(planes, G.IL, ld=64)
    # include/tvr.h: column c of plane p is half (c / 32) * 64 + p * 32 + c % 32 of the row
    for c_, p in ((0, 0), (31, 1), (32, 0), (63, 1)):
        assert il[3, (c_ // 32) * 64 + p * 32 + c_ % 32] == planes[p, 3, c_]
    assert np.isnan(G.plane_values(np.uint16([0x7E00]), G.X2F16)).all()
    assert np.isnan(G.plane_values(np.uint16([0x7FC0]), G.BF16)).all()
    v = np.float32([1.0, -2.5, 3.0e-5, 1234.567, 0.1])
    assert np.array_equal(G.bf16_bits(v), torch.from_numpy(v).bfloat16().view(torch.int16).numpy().view(np.uint16))


def test_raster_covers_every_tile_once():
    for M, N in ((300, 260), (513, 4352), (513, 516), (1, 4), (1300, 300)):
        nbm, nbn = G.tile_grid(M, N)
        seen = [G.tile_coords(t, M, N) for t in range(nbm * nbn)]
        assert sorted(seen) == sorted((i * 256, j * 256) for i in range(nbm) for j in range(nbn))
        assert G.tile_mask(M, N, 0, nbm * nbn).all() and not G.tile_mask(M, N, 0, 0).any()
    assert G.group_m(4352) == 4 and G.group_m(4096) == 2 and (3 * 17) % 8 != 0  # M = 513: 51 tiles


# ------------------------------------------------------------------ the ABI of tvr_gemm_launch
def test_header_struct_and_binding_agree():
    text = (ROOT / "include" / "tvr.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+tvr_gemm_launch\s*\(\s*tvr_model\s*\*\s*model\s*,\s*const\s+tvr_gemm_args\s*\*\s*args\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    body = re.search(r"typedef struct tvr_gemm_args \{(.*?)\} tvr_gemm_args;", code, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = ("ptr" if "*" in decl else "f32" if decl.startswith("float") else
                 "u64" if decl.startswith("uint64_t") else "i32")
        assert ctype != "i32" or decl.startswith("int32_t")
        names = re.sub(r"^(const\s+)?\w+\s*\*?", "", decl)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    kinds = {ctypes.c_int32: "i32", ctypes.c_float: "f32", ctypes.c_uint64: "u64", ctypes.c_void_p: "ptr"}
    assert fields == [(n, kinds[t]) for n, t in L.CGemmArgs._fields_]
    assert ctypes.sizeof(L.CGemmArgs) == 24 * 4 + 8 + 8 + 12 * 8 and L.CGemmArgs.wps.offset == 104
    for name, value in (("TVR_EPI_BIAS", L.EPI_BIAS), ("TVR_EPI_GELU", L.EPI_GELU), ("TVR_EPI_RESID", L.EPI_RESID),
                        ("TVR_FORM_PLAN", L.FORM_PLAN), ("TVR_FORM_PLAIN", L.FORM_PLAIN),
                        ("TVR_FORM_SPLITK", L.FORM_SPLITK), ("TVR_FORM_TAIL", L.FORM_TAIL),
                        ("TVR_FORM_STREAMK", L.FORM_STREAMK), ("TVR_SLICE_MODEL", L.SLICE_MODEL),
                        ("TVR_SLICE_ON", L.SLICE_ON), ("TVR_SLICE_OFF", L.SLICE_OFF)):
        assert re.search(rf"\b{name}\s*=\s*{value}\b", code)
    assert "#define TVR_ABI_VERSION 11" in text  # a backward-compatible addition
    assert hasattr(ctypes.CDLL(str(L.LIB_PATH)), "tvr_gemm_launch")
    res, args = L.SIGNATURES["tvr_gemm_launch"]
    assert res is ctypes.c_int and len(args) == 3 and L.load().tvr_abi_version() == L.ABI_VERSION == 11


def valid_args(**kw):
    """A launch that would be accepted: 300 x 260 x 512, x2f16, two planes, plain.  The buffers are host
    memory that no accepted launch ever sees: these tests only send refused ones."""
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 63) & ~63
    rows = (ctypes.c_int32 * 300)(*range(300))
    a = L.CGemmArgs(fmt=G.X2F16, exact16=0, epi=L.EPI_BIAS, form=L.FORM_PLAIN, form_n=0, form_tile=0,
                    slicing=L.SLICE_MODEL, skinny=0, M=300, N=260, K=512, lda=512, ldw=512, ld0=260, n_split=0,
                    ld1h=0, ps1h=0, raw_rows=0, ld_raw=0, mirror_rows=0, ldr=0, a2_col=0, a_buf_rows=0,
                    out_buf_rows=0, w_scale=1024.0, wps=512 * 260, A=p, a2=None, W=p, bias=p, out0=p, out0m=None,
                    out1h=None, raw=None, resid=None, range_flag=None, a_rows=None, out_rows=None)
    a._keep = (buf, rows)
    for k, v in kw.items():
        if k in ("a_rows", "out_rows") and v is not None:
            arr = (ctypes.c_int32 * len(v))(*v)
            a._keep += (arr,)
            v = ctypes.cast(arr, ctypes.c_void_p)
        if v == "p":
            v = p
        if v == "p+4":
            v = p + 4
        setattr(a, k, v)
    return a


GELU = dict(epi=1, n_split=128, out1h="p", ld1h=272, ps1h=136)
RESID = dict(epi=2, resid="p", ldr=260)
REFUSALS = {
    "unknown fmt": dict(fmt=1),
    "exact16 must": dict(exact16=2),
    "unknown epi": dict(epi=3),
    "unknown form": dict(form=5),
    "unknown slicing": dict(slicing=3),
    "skinny must": dict(skinny=2),
    "one exact fp16 weight plane": dict(fmt=G.BF16, exact16=1),
    "must be positive": dict(M=0),
    "must be positive ": dict(N=-1),
    "k-tile (32)": dict(K=48, lda=48, ldw=48),
    "k-tile (64)": dict(fmt=G.BF16, K=96, lda=96, ldw=96),
    "null A, W or out0": dict(A=None),
    "null A, W or out0 ": dict(W=None),
    "null A, W or out0  ": dict(out0=None),
    "w_scale": dict(w_scale=0.0),
    "w_scale ": dict(w_scale=float("inf")),
    "lda must": dict(lda=504),
    "lda must ": dict(lda=516),
    "lda must  ": dict(fmt=G.IL, exact16=1, lda=520),
    "ldw must": dict(ldw=516),
    "ldw must ": dict(ldw=256),
    "wps must": dict(wps=512 * 259),
    "wps must ": dict(wps=512 * 260 + 4),
    "ld0 must": dict(ld0=256),
    "16-byte aligned": dict(A="p+4"),
    "16-byte aligned ": dict(out0="p+4"),
    "16-byte aligned  ": dict(out0m="p+4"),
    "out_buf_rows must": dict(out_rows=list(range(300)), out_buf_rows=299),
    "out_rows[299] outside": dict(out_rows=list(range(299)) + [300], out_buf_rows=300),
    "out_rows[0] outside": dict(out_rows=[-1] + list(range(1, 300)), out_buf_rows=300),
    "names row 7 twice": dict(out_rows=list(range(299)) + [7], out_buf_rows=400),
    "a_buf_rows must": dict(a_rows=[0] * 300, a_buf_rows=0),
    "a_rows[5] outside": dict(a_rows=[0] * 5 + [9] + [0] * 294, a_buf_rows=9),
    "a2_col must": dict(a2="p", a2_col=128),
    "a2_col must ": dict(a2="p", a2_col=-256),
    "needs resid": dict(epi=2, ldr=260),
    "ldr must": dict(RESID, ldr=256),
    "no mirror": dict(RESID, out0m="p", mirror_rows=1),
    "mirror_rows outside": dict(out0m="p", mirror_rows=301),
    "mirror_rows outside ": dict(out0m="p", mirror_rows=-1),
    "n_split outside": dict(GELU, n_split=264),
    "needs out1h": dict(GELU, out1h=None),
    "too small for the GELU": dict(GELU, ps1h=128),
    "too small for the GELU ": dict(GELU, ld1h=264),
    "too small for the GELU  ": dict(GELU, fmt=G.IL, exact16=1, ld1h=256),
    "multiples of 8": dict(GELU, n_split=132),
    "multiples of 8 ": dict(GELU, ps1h=140, ld1h=280 - 4),
    "not with out_rows": dict(GELU, raw="p", raw_rows=1, ld_raw=132, out_rows=list(range(300)), out_buf_rows=300),
    "raw_rows outside": dict(GELU, raw="p", raw_rows=301, ld_raw=132),
    "ld_raw must": dict(GELU, raw="p", raw_rows=1, ld_raw=128),
    "ld_raw must ": dict(GELU, raw="p", raw_rows=1, ld_raw=134),
    "plain bias launch only": dict(fmt=G.IL, epi=2, resid="p", ldr=260),
    "plain bias launch only ": dict(fmt=G.IL, form=2, form_n=2),
    "plain bias launch only  ": dict(fmt=G.IL, skinny=1),
    "skinny is an opt-in": dict(skinny=1, form=2, form_n=2),
    "skinny is an opt-in ": dict(skinny=1, out0m="p", mirror_rows=1),
    "skinny is an opt-in  ": dict(RESID, skinny=1),
    "needs the vector epilogue": dict(form=2, form_n=2, N=258, ld0=260, wps=512 * 260),
    "needs the vector epilogue ": dict(form=4, form_n=4, ld0=262),
    "form_tile outside": dict(form=3, form_n=2, form_tile=0),
    "form_tile outside ": dict(form=3, form_n=2, form_tile=4),
    "form_tile outside  ": dict(form=4, form_n=4, form_tile=4),
    "form_tile outside   ": dict(form=4, form_n=4, form_tile=-1),
    "at least 8 k-tiles": dict(form=2, form_n=3),
    "at least 8 k-tiles ": dict(form=2, form_n=1),
    "at least 8 k-tiles  ": dict(form=3, form_tile=1, form_n=0),
    "workspace cap": dict(form=2, form_n=2, M=256 * 40, N=256 * 52, wps=512 * 256 * 52, ld0=256 * 52),
    "stream-K blocks": dict(form=4, form_n=3),
    "stream-K blocks ": dict(form=4, form_n=257, K=32 * 100, lda=3200, ldw=3200, wps=3200 * 260),
    "stream-K blocks  ": dict(form=4, form_tile=3, form_n=17),
}


def test_every_refusal_is_invalid_before_the_model_is_read():
    lib = L.load()
    assert lib.tvr_gemm_launch(None, ctypes.byref(valid_args()), None) == L.TVR_ERR_INVALID
    assert lib.tvr_last_error().startswith(b"tvr_gemm_launch: null model")
    # any non-null address stands in for the model: every refusal returns before the model is read
    fake = (ctypes.c_char * 64)()
    model = ctypes.addressof(fake)
    assert lib.tvr_gemm_launch(model, None, None) == L.TVR_ERR_INVALID
    assert lib.tvr_last_error().startswith(b"tvr_gemm_launch: null args")
    for what, kw in REFUSALS.items():
        rc = lib.tvr_gemm_launch(model, ctypes.byref(valid_args(**kw)), None)
        msg = lib.tvr_last_error().decode()
        assert rc == L.TVR_ERR_INVALID and what.strip() in msg, (what, kw, rc, msg)
    assert bytes(fake) == bytes(64)
