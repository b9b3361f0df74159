"""Per-source-token logit attribution on the GPU: ``head_direction_kernel`` alone
(``tvr_head_directions``), ``source_attribution_kernel`` alone
(``tvr_attention_source``), on a trace (``tvr_trace_source_attribution``) and
through the façade (``head_source_attribution``), against the fp64 references of
tests/source_cases.py and the fp64 oracle.

G pass: one small two-layer model per (d_head, n_heads) of attention_cases.MODELS,
its layer-1 W_O the operand; n = 1 / 15 / 16 / 17 / 33 rows into NaN-guarded
buffers (nothing outside [n][d] is written), NaN rows of dirs beyond n that must
not reach any output; against fp64 at source_cases.g_bar (4 x the larger error of
two fp32 products, floored at 4 x 2^-24 x the largest sum of |terms|); unit rows of
dirs give the rows of W_O bit for bit; each row alone has the bits it has inside
n = 33; a second run gives identical bits.

Source kernel: T = 1 / 15 / 63 / 64 / 65 / 129, every kind of source_cases at its
bar; ``unit`` is tvr_attention_pattern's output on the same buffer bit for bit,
``select`` the exact product at the hot key and zero elsewhere, ``zero`` exactly 0;
columns (q, ld) are +0.0; the outputs sit 4 bytes off a 16-byte boundary between
untouched guards; out_src has the same bits with and without out_cls; with every
key its own class out_cls equals out_src; a class without keys gives +0.0; each
sequence launched alone equals the batch; a repeat run gives identical bits; every
refusal of the header behind a real model.

Trace path: tiny model on f32 / x2f16 / x3bf16 and an exact-fp16 model, out_src
against the fp64 reference built from the trace's OWN exported hook_q / hook_k /
hook_v, final residual and fp32 weights, at source_cases.bar plus the rotary-table
allowance of test_gpu_attention_pattern.py (2 x the table shift of the pattern,
times the largest |v . g|); a pending (deferred) trace gives the bits of a filled
one; mid-sequence positions; one layer per group (TVR_SOURCE_G_MB=0) gives the
bits of one group.

End to end against the fp64 oracle at max(4 x |fp32 oracle - fp64 oracle|, floor),
floor 4 x 2^-24 x the largest sum of |terms| of an output.  Conservation: the sum
over keys of out_src (in fp64 on the host) against the engine's own out_head at
the SUM of the two oracle bars (that of the summed sources and that of the heads):
each side is held to the oracle by its own bar, and in the oracle they are equal.

Measured on an MI355X by this file (worst err / bar, printed at its end).
G pass, worst over the kinds, n = 1 / 15 / 16 / 17 / 33:
  d_head  16: 0.178 0.129 0.110 0.124 0.149
  d_head  64: 0.119 0.111 0.105 0.081 0.098
  d_head  80: 0.124 0.083 0.096 0.137 0.081
  d_head 128: 0.156 0.096 0.108 0.117 0.117
(layer 0: at most 0.130); unit rows of dirs bitwise.  Source kernel, worst over
the kinds and both ld, T = 1 / 15 / 63 / 64 / 65 / 129:
  d_head  16: 0.122 0.233 0.190 0.167 0.164 0.191
  d_head  64: 0.061 0.160 0.182 0.082 0.179 0.100
  d_head  80: 0.062 0.121 0.110 0.159 0.178 0.238
  d_head 128: 0.175 0.303 0.223 0.199 0.336 0.186
select and unit bitwise at every d_head.  Trace against its own rows: f32 0.085,
x2f16 0.064, x3bf16 0.135, exact-fp16 0.064.  End to end against the fp64 oracle:
f32 0.286, x2f16 0.251, x3bf16 0.235; conservation against out_head 0.047 / 0.063 /
0.078.  Façade: head_source_attribution 0.028 / 0.033 / 0.017, its sum over roles
against head_logit_attribution's heads 0.009 / 0.011 / 0.011.  The whole file (64
tests) runs in about 2.4 s.
"""
import collections
import functools
import gc
import math
import os
import random
import time

import numpy as np
import pytest
import torch

import attention_cases as A
import attribution_cases as C
import pattern_cases as P
import source_cases as S
import tvr_amd
from conftest import make_oracle
from tvr_amd import _lib as L, experiments
from tvr_amd.prompts import ROLES

pytestmark = [pytest.mark.gpu]

G = 2                  # guard rows before and after every output
NAN_BITS = 0x7FC00000  # torch.full(nan)
EPS24 = 2.0 ** -24
MODEL_IDS = [f"dh{dh}h{h}" for dh, h in A.MODELS]
ARROW = tvr_amd.tasks.ARROW
LENS = (1, 5, 17, 33)
MID = (0, 2, 8, 20)
TARGETS = (5, 77, 300, 41)
CONTRAST = (9, 3, 411, 200)

_worst = collections.defaultdict(float)


def note(form, err, bar):
    _worst[form] = max(_worst[form], err / bar if bar > 0 else (0.0 if err == 0 else float("inf")))
    return err <= bar


@pytest.fixture(scope="module", autouse=True)
def _module():
    t0 = time.time()
    yield
    for form, r in sorted(_worst.items()):
        print(f"\nsource attribution, worst err / bar: {form:44s} {r:.3f}", end="")
    print(f"\nsource attribution tests: {time.time() - t0:.1f} s from the first test to the last")
    for cache in (_ref, _ctx):
        cache.cache_clear()
    _oracle_cache.clear()
    gc.collect()
    torch.cuda.empty_cache()


class Ctx:
    def __init__(self, DH, H):
        self.DH, self.H, self.d = DH, H, DH * H
        cfg = tvr_amd.config.PythiaConfig(2, self.d, H, C.D_MLP, 64, n_ctx=A.N_CTX, name=f"source-{DH}x{H}")
        w = tvr_amd.weights.synth_engine_weights(cfg, seed=1, device="cuda", std=0.2)
        self.model = tvr_amd.Model(cfg, w, tokenizer=tvr_amd.tokenizer.SyntheticTokenizer(512), device="cuda", gemm="f32")
        self.lib, self.h = self.model._lib, self.model._h
        self.W = [lay.w2.cpu().numpy() for lay in w.layers]
        self.cos, self.sin = A.tables(DH, A.N_CTX)
        self.d_cos, self.d_sin = torch.from_numpy(self.cos).cuda(), torch.from_numpy(self.sin).cuda()

    def stream(self):
        return self.model._stream()


@functools.lru_cache(maxsize=None)  # one model per (d_head, n_heads) for the module: _module clears it
def _ctx(model):
    return Ctx(*model)


@pytest.fixture(params=A.MODELS, ids=MODEL_IDS)
def ctx(request):
    return _ctx(request.param)


@functools.lru_cache(maxsize=None)
def _ref(model, kind, T):
    """(case, src64, bar): computed once, shared by every test and left unchanged."""
    c = _ctx(model)
    case = S.make(kind, model[0], model[1], T, W=c.W[1])
    ref = S.reference(case, c.cos, c.sin)
    return case, ref, S.bar(case, c.cos, c.sin, ref)[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def nan_padded(a, extra=2):
    """a [n][d] on the device with ``extra`` NaN rows behind it (16-byte aligned: a fresh allocation)."""
    t = torch.full((a.shape[0] + extra, a.shape[1]), float("nan"), dtype=torch.float32, device="cuda")
    t[:a.shape[0]] = torch.from_numpy(a)
    return t


class Guarded:
    """A NaN-filled float buffer with an array of ``shape`` inside it, G rows of guard on either side, starting
    ``shift`` floats into the allocation (shift = 1: 4-byte aligned only)."""

    def __init__(self, shape, shift=1):
        self.shape, self.shift = tuple(shape), shift
        self.size, row = int(np.prod(shape)), int(np.prod(shape[1:]))
        self.t = torch.full((self.size + 2 * G * row + 4,), float("nan"), dtype=torch.float32, device="cuda")
        self.at = shift + G * row
        self.ptr = self.t.data_ptr() + 4 * self.at
        assert shift == 0 or self.ptr % 16 != 0  # (4-byte aligned only)

    def read(self, what):
        h = self.t.cpu().numpy()
        b = h.view(np.int32)
        inside = np.zeros(h.shape, dtype=bool)
        inside[self.at:self.at + self.size] = True
        assert (b[~inside] == NAN_BITS).all(), f"{what}: written outside its array"
        return h[inside].reshape(self.shape).copy()

    def untouched(self):
        return (self.t.cpu().numpy().view(np.int32) == NAN_BITS).all()


# ------------------------------------------------------------------------------ 1: the G pass
def run_g(ctx, dirs_dev, n, layer=1):
    """One tvr_head_directions launch over the first n rows: out_g [n][d]."""
    out = Guarded((n, ctx.d), shift=0)  # (the entry point wants 16-byte aligned buffers)
    rc = ctx.lib.tvr_head_directions(ctx.h, layer, dirs_dev.data_ptr(), n, out.ptr, ctx.stream())
    L.check(rc, "tvr_head_directions")
    torch.cuda.synchronize()
    got = out.read("out_g")
    assert not np.isnan(got).any(), "NaN in G: a row of dirs beyond n was read"
    return got


def test_g_pass_against_fp64(ctx):
    model = (ctx.DH, ctx.H)
    for n in C.ALL_N:
        for kind in ("random", "gain", "select"):
            dirs = C.make(kind, ctx.DH, ctx.H, n, W=ctx.W[1]).dirs
            dev = nan_padded(dirs)
            ref = S.g_of(dirs, ctx.W[1])
            bar = S.g_bar(dirs, ctx.W[1], ref)[0]
            got = run_g(ctx, dev, n)
            err = S.max_err(got, ref)
            ok = note(f"G pass d_head {ctx.DH:3d} n {n:2d}", err, bar)
            print(f"head directions {model} {kind:6s} n {n:2d}: err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
            assert ok, (model, kind, n, err, bar)
            assert (bits(run_g(ctx, dev, n)) == bits(got)).all(), "a second run gives other bits"
            if kind == "select":  # dirs = e_c: the row c of W_O, bit for bit
                c = np.argmax(dirs, -1)
                assert (bits(got) == bits(ctx.W[1][c, :ctx.d])).all(), (model, n)


def test_g_pass_layer_and_row_independence(ctx):
    case = C.make("gain", ctx.DH, ctx.H, 33, W=ctx.W[1])
    dev = nan_padded(case.dirs)
    full = run_g(ctx, dev, 33)
    for n in (1, 16, 17):  # a prefix of the rows: another chunk count, another last-chunk mask
        assert (bits(run_g(ctx, dev, n)) == bits(full[:n])).all(), n
    for i in range(33):  # each row alone (16-byte aligned: a row is d floats)
        one = nan_padded(case.dirs[i:i + 1])
        assert (bits(run_g(ctx, one, 1)) == bits(full[i:i + 1])).all(), i
    ref0 = S.g_of(case.dirs, ctx.W[0])
    bar0 = S.g_bar(case.dirs, ctx.W[0], ref0)[0]
    assert note(f"G pass d_head {ctx.DH:3d} layer 0", S.max_err(run_g(ctx, dev, 33, layer=0), ref0), bar0)
    assert S.max_err(full, ref0) > 100 * bar0  # (the other layer's W_O is another matrix)
    # the façade: the same kernel through the operator
    t = torch.from_numpy(case.dirs).cuda()
    assert (bits(ctx.model.head_directions(1, t).cpu().numpy()) == bits(full)).all()
    assert (bits(ctx.model.head_directions(1, t[1:]).cpu().numpy()) == bits(full[1:])).all()


def test_invalid_direction_arguments_launch_nothing():
    ctx = _ctx(A.MODELS[0])
    dirs = nan_padded(C.make("random", ctx.DH, ctx.H, 17, W=ctx.W[1]).dirs)
    ref = run_g(ctx, dirs, 17)
    out = Guarded((17, ctx.d), shift=0)
    dp = dirs.data_ptr()

    def refused(message, layer, dirs_p, n, out_p, model=ctx.h):
        rc = ctx.lib.tvr_head_directions(model, layer, dirs_p, n, out_p, ctx.stream())
        err = ctx.lib.tvr_last_error().decode()
        assert rc == L.TVR_ERR_INVALID and err.startswith("tvr_head_directions: ") and message in err, (message, rc, err)

    refused("null model", 1, dp, 17, out.ptr, model=None)
    refused("null argument", 1, None, 17, out.ptr)
    refused("null argument", 1, dp, 17, None)
    refused("n must be positive", 1, dp, 0, out.ptr)
    refused("n must be positive", 1, dp, -3, out.ptr)
    refused("layer out of range", -1, dp, 17, out.ptr)
    refused("layer out of range", 2, dp, 17, out.ptr)
    refused("16-byte aligned", 1, dp + 4, 16, out.ptr)
    refused("16-byte aligned", 1, dp, 16, out.ptr + 8)
    torch.cuda.synchronize()
    assert out.untouched()
    L.check(ctx.lib.tvr_head_directions(ctx.h, 1, dp, 17, out.ptr, ctx.stream()), "tvr_head_directions")
    torch.cuda.synchronize()
    assert (bits(out.read("out_g")) == bits(ref)).all()  # the model is still usable


# ------------------------------------------------------------------------------ 2: the source kernel
def to_device(case):
    if not hasattr(case, "dev"):  # the inputs go to the device once per case
        case.dev = torch.from_numpy(case.qkv).cuda()
        case.gdev = nan_padded(case.g)


def call(ctx, case, cls, n_classes, src, ld, cls_out, tables=True, qkv=None, rows=None, row0=None, qpos=None, n_seq=None,
         g=None):
    """tvr_attention_source with the case's arguments, any of them overridden; returns the status."""
    to_device(case)
    row0 = case.row0 if row0 is None else np.asarray(row0, dtype=np.int32)
    qpos = case.qpos if qpos is None else np.asarray(qpos, dtype=np.int32)
    cls = None if cls is None else np.ascontiguousarray(cls, dtype=np.int32)
    return ctx.lib.tvr_attention_source(
        ctx.h, case.dev.data_ptr() if qkv is None else qkv, case.lay.rows if rows is None else rows,
        row0.ctypes.data, qpos.ctypes.data, case.lay.n_seq if n_seq is None else n_seq,
        case.gdev.data_ptr() if g is None else g, None if cls is None else cls.ctypes.data, n_classes, src, ld, cls_out,
        ctx.d_cos.data_ptr() if tables else None, ctx.d_sin.data_ptr() if tables else None, ctx.stream())


def run(ctx, case, ld=None, cls=None, n_classes=0, want_src=True, want_cls=False, seq=None):
    """One launch on guarded, NaN-filled outputs 4 bytes off a 16-byte boundary: (src [n_seq][H][ld] or None,
    by class [n_seq][H][C] or None).  seq: that sequence alone (its own descriptors and row of g).  Asserts the
    guards, no NaN, and +0.0 in the columns beyond every query position."""
    to_device(case)
    H = case.n_heads
    qpos = case.qpos if seq is None else case.qpos[seq:seq + 1]
    n = len(qpos)
    ld = case.maxT if ld is None else ld
    src = Guarded((n, H, ld)) if want_src else None
    out_cls = Guarded((n, H, n_classes)) if want_cls else None
    kw = {} if seq is None else dict(row0=case.row0[seq:seq + 1], qpos=qpos, n_seq=1,
                                     g=case.gdev.data_ptr() + 4 * case.d * seq)
    rc = call(ctx, case, cls, n_classes, None if src is None else src.ptr, ld, None if out_cls is None else out_cls.ptr, **kw)
    L.check(rc, "tvr_attention_source")
    a = b = None
    if src is not None:
        a = src.read("out_src")
        assert not np.isnan(a).any(), "NaN in out_src: a row, a Q or a V that is not the sequence's was read"
        for s, q in enumerate(qpos):
            assert (bits(a[s, :, q + 1:]) == 0).all(), "columns (qpos, ld) must be +0.0"
    if out_cls is not None:
        b = out_cls.read("out_cls")
        assert not np.isnan(b).any(), "NaN in out_cls"
    return a, b


def pattern_of(ctx, case, ld):
    """tvr_attention_pattern's output on the same buffer."""
    to_device(case)
    out = Guarded((case.lay.n_seq, case.n_heads, ld))
    rc = ctx.lib.tvr_attention_pattern(ctx.h, case.dev.data_ptr(), case.lay.rows, case.row0.ctypes.data,
                                       case.qpos.ctypes.data, case.lay.n_seq, None, 0, out.ptr, ld, None,
                                       ctx.d_cos.data_ptr(), ctx.d_sin.data_ptr(), ctx.stream())
    L.check(rc, "tvr_attention_pattern")
    return out.read("out_pattern")


def test_source_kernel_against_fp64(ctx):
    model = (ctx.DH, ctx.H)
    for T in S.ALL_T:
        for kind in S.KINDS:
            case, ref, bar = _ref(model, kind, T)
            for ld in (T, T + 3):
                got, _ = run(ctx, case, ld=ld)
                err = S.max_err(got[..., :T], ref)
                ok = note(f"source kernel d_head {ctx.DH:3d} T {T:3d}", err, bar)
                print(f"attention source {model} {kind:11s} T {T:3d} ld {ld:3d}: err {err:.3e} bar {bar:.3e}")
                assert ok, (model, kind, T, ld, err, bar)
            again, _ = run(ctx, case, ld=T + 3)
            assert (bits(again) == bits(got)).all(), "a repeat run gives other bits"
            if kind == "unit":  # every v . g is exactly 1.0: the pattern, bit for bit
                assert (bits(got) == bits(pattern_of(ctx, case, T + 3))).all(), (model, T)
            if kind == "zero":
                assert (got == 0).all(), (model, T)
            for s in range(case.lay.n_seq):  # each sequence launched alone equals the batch
                alone, _ = run(ctx, case, ld=T + 3, seq=s)
                assert (bits(alone[0]) == bits(got[s])).all(), (model, kind, T, s)


def test_select_is_exact(ctx):
    """One exact product at the hot key (bit for bit), zero elsewhere, for every rotation of the select families."""
    for T in S.ALL_T:
        for rot in A.SELECT_ROTS:
            case = S.make("select", ctx.DH, ctx.H, T, rot=rot)
            got, _ = run(ctx, case, ld=T + 1)
            want = S.select_exact(case, T + 1)
            hot = want != 0
            assert (bits(got)[hot] == bits(want)[hot]).all() and (got[~hot] == 0).all(), (T, rot)
    _worst[f"source kernel d_head {ctx.DH:3d} select: bitwise"] = 0.0


def test_classes(ctx):
    model = (ctx.DH, ctx.H)
    NC = P.N_CLASSES
    for T in S.ALL_T:
        case, _, _ = _ref(model, "random_gain", T)
        cls = S.classes(case)
        alone, _ = run(ctx, case)
        src, by = run(ctx, case, cls=cls, n_classes=NC, want_cls=True)
        assert (bits(src) == bits(alone)).all(), "asking for out_cls changed out_src"
        want = S.class_sums(src, case, cls)
        mags = S.class_sums(np.abs(src), case, cls)
        for s, q in enumerate(case.qpos):  # any-order fp32 summation of q + 1 terms
            assert (np.abs(by[s].astype(np.float64) - want[s]) <= (q + 1) * EPS24 * mags[s] + 1e-45).all(), (T, s)
        empty = mags == 0  # no key of the class among the seen ones (src is not 0 for a seen key of these cases)
        assert empty[1, :, 2].all() and empty[2, :, 0].all() and empty[2, :, 2].all()
        assert (bits(by)[empty] == 0).all(), "a class without keys must be +0.0"
        src2, by2 = run(ctx, case, cls=cls, n_classes=NC, want_cls=True)
        assert (bits(src2) == bits(src)).all() and (bits(by2) == bits(by)).all(), "two runs differ"
        _, by3 = run(ctx, case, cls=cls, n_classes=NC, want_src=False, want_cls=True)
        assert (bits(by3) == bits(by)).all(), "out_cls depends on whether out_src is written"
        src4, _ = run(ctx, case, cls=cls, n_classes=NC)  # the classes given but no sums asked for
        assert (bits(src4) == bits(src)).all()
        if T <= L.PATTERN_MAX_CLASSES:  # every key its own class: out_cls is out_src (one term per sum)
            own = np.full(case.lay.rows, -1, dtype=np.int32)
            for sd in case.seqs:
                own[sd.row0:sd.row0 + sd.n] = np.arange(sd.n)
            src5, by5 = run(ctx, case, cls=own, n_classes=T, want_cls=True)
            assert np.array_equal(by5, src5[..., :T]), (T,)  # (numerically: 0 + -0.0 is +0.0)
            assert (bits(src5) == bits(src)).all()


def test_model_tables(ctx):
    """cos_t = sin_t = NULL (the model's own tables): tvr_attention_pattern's allowance, times the largest |v . g|."""
    case, ref, bar = _ref((ctx.DH, ctx.H), "random", 129)
    to_device(case)
    out = Guarded((case.lay.n_seq, ctx.H, 129))
    L.check(call(ctx, case, None, 0, out.ptr, 129, None, tables=False), "tvr_attention_source")
    dots = np.abs(S.dots_given(case, np.float64)).max()
    assert S.max_err(out.read("out_src"), ref) <= bar + 2 * table_shift(case, ctx.DH) * dots


def table_shift(case, DH, n_ctx=A.N_CTX):
    """What moving TL's fp32 frequencies by 2 ulp does to the fp64 pattern of the case."""
    f = A.tl_freq32(DH)
    pa = P.reference(case, *A.tables_from_freq(f, n_ctx))
    pb = P.reference(case, *A.tables_from_freq(f * (1 + 2.0 ** -22), n_ctx))
    return P.max_err(pb, pa)


def test_invalid_source_arguments_launch_nothing():
    ctx = _ctx(A.MODELS[0])
    case, _, _ = _ref(A.MODELS[0], "random", 17)
    n, H, T, NC = case.lay.n_seq, ctx.H, 17, P.N_CLASSES
    cls = S.classes(case)
    src, by = Guarded((n, H, T)), Guarded((n, H, NC))
    so, co = src.ptr, by.ptr
    want, want_by = run(ctx, case, cls=cls, n_classes=NC, want_cls=True)  # (the inputs are on the device from here on)
    qkv, g = case.dev.data_ptr(), case.gdev.data_ptr()

    def refused(message, *a, **kw):
        rc = call(ctx, case, *a, **kw)
        err = ctx.lib.tvr_last_error().decode()
        assert rc == L.TVR_ERR_INVALID and err.startswith("tvr_attention_source: ") and message in err, (message, rc, err)

    bad_cls = cls.copy()
    bad_cls[case.row0[0] + 3] = NC
    low_cls = cls.copy()
    low_cls[0] = -2
    refused("null qkv", cls, NC, so, T, co, qkv=0)
    refused("null g", cls, NC, so, T, co, g=0)
    refused("both null", cls, NC, None, T, None)
    refused("out_cls needs cls", None, NC, so, T, co)
    refused("n_classes must be in [1, 64]", cls, 0, so, T, co)
    refused("n_classes must be in [1, 64]", cls, 65, so, T, None)
    refused("outside [-1, n_classes)", bad_cls, NC, so, T, co)
    refused("outside [-1, n_classes)", low_cls, NC, so, T, None)
    refused("n_seq must be positive", cls, NC, so, T, co, n_seq=0)
    refused("rows must be positive", cls, NC, so, T, co, rows=0)
    refused("qpos outside [0, n_ctx)", cls, NC, so, T, co, qpos=[-1, 8, 0])
    refused("qpos outside [0, n_ctx)", cls, NC, so, A.N_CTX + 1, co, qpos=[A.N_CTX, 8, 0])
    refused("ld must exceed", cls, NC, so, T - 1, co)
    refused("outside the qkv buffer", cls, NC, so, T, co, row0=[-1, 19, 37])
    refused("outside the qkv buffer", cls, NC, so, T, co, rows=int(case.row0[2]))
    refused("16-byte aligned", cls, NC, so, T, co, qkv=qkv + 4)
    refused("16-byte aligned", cls, NC, so, T, co, g=g + 8)
    rc = ctx.lib.tvr_attention_source(ctx.h, qkv, case.lay.rows, case.row0.ctypes.data, case.qpos.ctypes.data, n, g, None, 0,
                                      so, T, None, ctx.d_cos.data_ptr(), None, ctx.stream())
    assert rc == L.TVR_ERR_INVALID and "cos_t and sin_t" in ctx.lib.tvr_last_error().decode()
    rc = ctx.lib.tvr_attention_source(ctx.h, qkv, case.lay.rows, None, case.qpos.ctypes.data, n, g, None, 0, so, T, None,
                                      None, None, ctx.stream())
    assert rc == L.TVR_ERR_INVALID and "null row0 / qpos" in ctx.lib.tvr_last_error().decode()
    rc = ctx.lib.tvr_attention_source(None, qkv, case.lay.rows, case.row0.ctypes.data, case.qpos.ctypes.data, n, g, None, 0,
                                      so, T, None, None, None, ctx.stream())
    assert rc == L.TVR_ERR_INVALID and "null model" in ctx.lib.tvr_last_error().decode()
    torch.cuda.synchronize()
    assert src.untouched() and by.untouched()
    # ld is not looked at when out_src is not asked for; and the model is still usable
    assert call(ctx, case, cls, NC, None, 0, co) == L.TVR_OK
    assert (bits(by.read("out_cls")) == bits(want_by)).all()
    # the operator: the same kernel, the same bits
    o_src = torch.full((n, H, T), float("nan"), device="cuda")
    ctx.model._ops.attention_source(ctx.h.value, case.dev, torch.from_numpy(case.row0), torch.from_numpy(case.qpos),
                                    case.gdev[:n], None, 0, ctx.d, H, o_src, None, ctx.d_cos, ctx.d_sin)
    assert (bits(o_src.cpu().numpy()) == bits(want)).all()
    with pytest.raises(ValueError, match=r"\[n_seq, d_model\]"):
        ctx.model._ops.attention_source(ctx.h.value, case.dev, torch.from_numpy(case.row0), torch.from_numpy(case.qpos),
                                        case.gdev[:n, :ctx.d - 16].contiguous(), None, 0, ctx.d, H, o_src, None, None, None)


def test_too_many_keys_are_unsupported_before_any_launch():
    """(2 d_head + keys) floats beyond 64 KiB: TVR_ERR_UNSUPPORTED, nothing written (the buffers are real and hold
    every row the descriptors name)."""
    DH, H, n_ctx = 16, 4, 16400
    cfg = tvr_amd.config.PythiaConfig(1, DH * H, H, C.D_MLP, 64, n_ctx=n_ctx, name="source-long")
    w = tvr_amd.weights.synth_engine_weights(cfg, seed=1, device="cuda")
    m = tvr_amd.Model(cfg, w, tokenizer=tvr_amd.tokenizer.SyntheticTokenizer(512), device="cuda", gemm="f32")
    qkv = torch.zeros(n_ctx, 3 * DH * H, device="cuda")
    g = torch.zeros(1, DH * H, device="cuda")
    out = Guarded((1, H, 1))
    cls = np.zeros(n_ctx, dtype=np.int32)
    row0 = np.zeros(1, dtype=np.int32)

    def status(keys):
        qpos = np.asarray([keys - 1], dtype=np.int32)
        return m._lib.tvr_attention_source(m._h, qkv.data_ptr(), n_ctx, row0.ctypes.data, qpos.ctypes.data, 1,
                                           g.data_ptr(), cls.ctypes.data, 1, None, 0, out.ptr, None, None, m._stream())

    rc = status(16384 - 2 * DH + 1)  # 64 KiB + 4 B
    err = m._lib.tvr_last_error().decode()
    assert rc == L.TVR_ERR_UNSUPPORTED and "do not fit" in err, (rc, err)
    torch.cuda.synchronize()
    assert out.untouched()
    assert status(16384 - 2 * DH) == L.TVR_OK  # exactly 64 KiB: V = 0, so every key's value is 0
    assert (out.read("out_cls") == 0).all()


# ------------------------------------------------------------------------------ 3: the trace path
def ragged_prompts(cfg, lens, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [[0] + torch.randint(1, cfg.d_vocab, (n - 1,), generator=g).tolist() for n in lens]


def filled_trace(model, seqs, defer=False):
    trace = model.trace(len(seqs), sum(map(len, seqs)))
    model.forward_clean(seqs, trace=trace, defer=defer)
    return trace


@pytest.fixture(scope="module")
def exact16_model(tiny_cfg, tokenizer):
    """fp16-valued weights: the exact-fp16 GEMMs are bound and the trace is uncentred (as
    tests/test_gpu_task_vectors.py builds its model)."""
    sd = tvr_amd.weights.synth_hf_state_dict(tiny_cfg, seed=0, std=0.3, fp16=True)
    m = tvr_amd.Model.from_hf_state_dict(tiny_cfg, sd, device="cuda", tokenizer=tokenizer, gemm="x2f16")
    assert m.exact16
    return m


def check_trace_path(model, name):
    cfg = model.cfg
    nl, H, DH = cfg.n_layers, cfg.n_heads, cfg.d_head
    seqs = ragged_prompts(cfg, LENS)
    cos, sin = A.tables(DH, n_ctx=cfg.n_ctx, base=cfg.rotary_base)
    trace = filled_trace(model, seqs)
    wu = model.weights.w_unembed_t.cpu().numpy()
    Ws = [lay.w2.cpu().numpy() for lay in model.weights.layers]
    qkv = [(trace.q(l).cpu().numpy(), trace.k(l).cpu().numpy(), trace.v(l).cpu().numpy()) for l in range(nl)]
    first = True
    for pos in (None, MID):
        qpos = [len(s) - 1 for s in seqs] if pos is None else list(pos)
        rows = torch.as_tensor([o + q for o, q in zip(trace.seq_offsets, qpos)], device=model.device)
        xL = trace.resid_pre(nl)[rows].cpu().numpy()
        for ct in (None, CONTRAST):
            u = wu[list(TARGETS)] - (0 if ct is None else wu[list(ct)])
            src, none = trace.source_attribution(list(TARGETS), contrast=ct, pos=pos, want_keys=True)
            assert none is None and tuple(src.shape) == (len(seqs), nl, H, max(qpos) + 1)
            got = src.cpu().numpy()
            assert not np.isnan(got).any()
            for l in range(nl):
                case = S.from_rows(*qkv[l], LENS, qpos, DH, H, Ws[l], u, xL=xL, eps=cfg.ln_eps)
                ref = S.reference_from_model(case, cos, sin)
                dots = np.abs(S.dots_plain(case, np.float64)).max()
                bar = S.bar(case, cos, sin, ref, given=False)[0] + 2 * table_shift(case, DH, cfg.n_ctx) * dots
                err = S.max_err(got[:, l], ref[..., :got.shape[-1]])
                ok = note(f"trace vs own rows {name}", err, bar)
                print(f"trace source attribution ({name}, pos {pos}, contrast {ct is not None}, layer {l}): "
                      f"err {err:.3e} bar {bar:.3e}")
                assert ok, (name, pos, ct, l, err, bar)
                for s, q in enumerate(qpos):
                    assert (bits(got[s, l, :, q + 1:]) == 0).all()
            again = model.source_attribution(trace, list(TARGETS), contrast=ct, positions=pos, want_keys=True)[0]
            assert (bits(again.cpu().numpy()) == bits(got)).all()  # reproducible
            if first:  # the deferred clean forward runs inside the call: the same bits as on the filled trace
                pending = filled_trace(model, seqs, defer=True)
                assert (bits(pending.source_attribution(list(TARGETS), contrast=ct, pos=pos, want_keys=True)[0]
                             .cpu().numpy()) == bits(got)).all()
                first = False
            # the class sums on the trace: its own sources' sums, classes as one list per sequence and flat
            classes = [[(j * 5 + s) % 4 - 1 for j in range(len(q))] for s, q in enumerate(seqs)]
            src2, by = trace.source_attribution(list(TARGETS), contrast=ct, pos=pos, classes=classes, n_classes=3,
                                                want_keys=True)
            assert (bits(src2.cpu().numpy()) == bits(got)).all()
            by = by.cpu().numpy()
            for s, q in enumerate(qpos):
                c = np.asarray(classes[s][:q + 1])
                for k in range(3):
                    terms = got[s, :, :, :q + 1].astype(np.float64)[..., c == k]
                    assert (np.abs(by[s, :, :, k] - terms.sum(-1)) <= (q + 1) * EPS24 * np.abs(terms).sum(-1) + 1e-45).all()
            flat = trace.source_attribution(list(TARGETS), contrast=ct, pos=pos, classes=[c for cs in classes for c in cs],
                                            n_classes=3)
            assert flat[0] is None and (bits(flat[1].cpu().numpy()) == bits(by)).all()
            # one layer per group: other launches, the same bits
            os.environ["TVR_SOURCE_G_MB"] = "0"
            try:
                split = trace.source_attribution(list(TARGETS), contrast=ct, pos=pos, classes=classes, n_classes=3,
                                                 want_keys=True)
            finally:
                del os.environ["TVR_SOURCE_G_MB"]
            assert (bits(split[0].cpu().numpy()) == bits(got)).all() and (bits(split[1].cpu().numpy()) == bits(by)).all()


def test_trace_path_against_its_own_rows(tiny_model):
    check_trace_path(tiny_model, tiny_model.gemm)


def test_trace_path_on_an_uncentred_trace(exact16_model):
    check_trace_path(exact16_model, "exact-fp16")


def test_trace_path_is_the_two_primitives(tiny_model):
    """One pair of kernels, two callers: tvr_head_directions and tvr_attention_source on the trace's exported rows,
    with the trace path's directions recovered as test_gpu_attribution.py recovers them."""
    cfg = tiny_model.cfg
    seqs = ragged_prompts(cfg, LENS)
    trace = filled_trace(tiny_model, seqs)
    src = trace.source_attribution(list(TARGETS), want_keys=True)[0].cpu().numpy()
    pat = trace.attention_pattern().cpu().numpy().astype(np.float64)
    rows = torch.as_tensor([o + n - 1 for o, n in zip(trace.seq_offsets, LENS)], device="cuda")
    xL = trace.resid_pre(cfg.n_layers)[rows]
    xc = xL - xL.mean(-1, keepdim=True)
    sigma = (xc.pow(2).mean(-1, keepdim=True) + cfg.ln_eps).sqrt()
    dirs = tiny_model.weights.w_unembed_t[list(TARGETS)] / sigma
    row0 = torch.as_tensor(trace.seq_offsets, dtype=torch.int32)
    qpos = torch.as_tensor([n - 1 for n in LENS], dtype=torch.int32)
    for l in range(cfg.n_layers):
        g = tiny_model.head_directions(l, dirs)
        qkv = torch.cat([trace.q(l), trace.k(l), trace.v(l)], 1).contiguous()
        out = torch.empty(len(seqs), cfg.n_heads, max(LENS), device="cuda")
        tiny_model._ops.attention_source(tiny_model._h.value, qkv, row0, qpos, g, None, 0, cfg.d_model, cfg.n_heads, out,
                                         None, None, None)
        # torch's mean / sqrt may differ from the kernel's by an ulp of sigma: 2^-22 relative to the sum of |terms|
        gn, vn = g.cpu().numpy().astype(np.float64), trace.v(l).cpu().numpy().astype(np.float64)
        for s, (o, n) in enumerate(zip(trace.seq_offsets, LENS)):
            terms = pat[s, l, :, :n] * np.einsum("jhe,he->hj", np.abs(vn[o:o + n]).reshape(n, cfg.n_heads, -1),
                                                 np.abs(gn[s]).reshape(cfg.n_heads, -1))
            diff = np.abs(out[s, :, :n].cpu().numpy().astype(np.float64) - src[s, l, :, :n])
            assert (diff <= 2.0 ** -21 * terms + 1e-45).all(), (l, s)


def test_invalid_trace_arguments_launch_nothing(tiny_model):
    cfg, lib, st = tiny_model.cfg, tiny_model._lib, tiny_model._stream()
    seqs = ragged_prompts(cfg, LENS)
    n, tokens, V = len(seqs), sum(LENS), cfg.d_vocab
    empty = tiny_model.trace(n, tokens)
    trace = filled_trace(tiny_model, seqs)
    ld, NC = max(LENS), 3
    src, by = Guarded((n, cfg.n_layers, cfg.n_heads, ld)), Guarded((n, cfg.n_layers, cfg.n_heads, NC))
    so, co = src.ptr, by.ptr
    cls = np.zeros(tokens, dtype=np.int32)
    tg, ct = np.asarray(TARGETS, dtype=np.int32), np.asarray(CONTRAST, dtype=np.int32)

    def p(a):
        return None if a is None else np.ascontiguousarray(a, dtype=np.int32)

    def refused(message, tr, pos, t, c, k, n_classes, sp, ldv, cp):
        arrs = [p(pos), p(t), p(c), p(k)]
        rc = lib.tvr_trace_source_attribution(tr._h, *[None if a is None else a.ctypes.data for a in arrs], n_classes, sp,
                                              ldv, cp, st)
        err = lib.tvr_last_error().decode()
        assert rc == L.TVR_ERR_INVALID and err.startswith("tvr_trace_source_attribution: ") and message in err, (message, rc, err)

    bad = cls.copy()
    bad[-1] = NC
    refused("null target", trace, None, None, ct, cls, NC, so, ld, co)
    refused("trace is empty", empty, None, tg, ct, cls, NC, so, ld, co)
    refused("both null", trace, None, tg, ct, cls, NC, None, ld, None)
    refused("out_cls needs cls", trace, None, tg, ct, None, NC, so, ld, co)
    refused("n_classes must be in [1, 64]", trace, None, tg, ct, cls, 0, so, ld, co)
    refused("n_classes must be in [1, 64]", trace, None, tg, ct, cls, 65, so, ld, co)
    refused("outside [-1, n_classes)", trace, None, tg, ct, bad, NC, so, ld, co)
    refused("pos of sequence 1 out of range", trace, [0, 5, 0, 0], tg, ct, cls, NC, so, ld, co)
    refused("pos of sequence 0 out of range", trace, [-1, 0, 0, 0], tg, ct, cls, NC, so, ld, co)
    refused("target of sequence 2 outside", trace, None, [1, 2, V, 3], ct, cls, NC, so, ld, co)
    refused("target of sequence 0 outside", trace, None, [-1, 2, 3, 3], None, cls, NC, so, ld, co)
    refused("contrast of sequence 3 outside", trace, None, tg, [1, 2, 3, V], cls, NC, so, ld, co)
    refused("contrast of sequence 1 outside", trace, None, tg, [1, -2, 3, 4], cls, NC, so, ld, None)
    refused("ld must exceed", trace, None, tg, ct, cls, NC, so, ld - 1, co)
    torch.cuda.synchronize()
    assert src.untouched() and by.untouched()
    # the façade's own checks come first and raise ValueError as well
    with pytest.raises(ValueError, match="outside its sequence"):
        trace.source_attribution(list(TARGETS), pos=[0, 5, 0, 0], want_keys=True)
    with pytest.raises(ValueError, match="trace is empty"):
        empty.source_attribution(list(TARGETS), want_keys=True)
    # afterwards the trace and the model are still usable: a valid call on the same buffers, offset outputs
    rc = lib.tvr_trace_source_attribution(trace._h, None, tg.ctypes.data, ct.ctypes.data, cls.ctypes.data, NC, so, ld, co, st)
    L.check(rc, "tvr_trace_source_attribution")
    torch.cuda.synchronize()
    want, want_by = trace.source_attribution(list(TARGETS), contrast=list(CONTRAST), classes=cls, n_classes=NC, want_keys=True)
    assert (bits(src.read("out_src")) == bits(want.cpu().numpy())).all()
    got_by = by.read("out_cls")
    assert (bits(got_by) == bits(want_by.cpu().numpy())).all() and (bits(got_by[..., 1:]) == 0).all()
    # ld is not looked at without out_src
    only = Guarded((n, cfg.n_layers, cfg.n_heads, NC))
    L.check(lib.tvr_trace_source_attribution(trace._h, None, tg.ctypes.data, ct.ctypes.data, cls.ctypes.data, NC, None, 0,
                                             only.ptr, st), "tvr_trace_source_attribution")
    torch.cuda.synchronize()
    assert (bits(only.read("out_cls")) == bits(got_by)).all()
    # a direct operator call with a wrong shape is refused before the engine is reached
    with pytest.raises(ValueError, match=r"\[n_seq, n_layers, n_heads, ld\]"):
        tiny_model._ops.source_attribution(trace._h.value, None, torch.from_numpy(tg), None, None, 0, n, cfg.n_layers,
                                           cfg.n_heads, torch.zeros(n, cfg.n_layers, cfg.n_heads + 1, ld, device="cuda"), None)
    with pytest.raises(ValueError, match="one entry per traced token"):
        tiny_model._ops.source_attribution(trace._h.value, None, torch.from_numpy(tg), None, torch.from_numpy(cls[:-1].copy()),
                                           NC, n, cfg.n_layers, cfg.n_heads, None,
                                           torch.zeros(n, cfg.n_layers, cfg.n_heads, NC, device="cuda"))


# ------------------------------------------------------------------------------ 4: against the oracle
def oracle_sources(o, ids, q, tg, ct):
    """In the oracle's dtype, as fp64 arrays: src [L][H][q + 1], heads [L][H] (hook_result . u / sigma), sums of
    |terms| of src [L][H][q + 1].  q / k / v recomputed from the cached hook_resid_pre as
    test_gpu_attention_pattern.oracle_qkv_pattern does."""
    nl, H, DH = o.cfg.n_layers, o.cfg.n_heads, o.cfg.d_head
    _, cache = o.run_with_cache(torch.tensor([ids]))
    xL = cache[f"blocks.{nl - 1}.hook_resid_post"][0, q]
    xc = xL - xL.mean()
    dirs = (o.w["W_U"][:, tg] - (o.w["W_U"][:, ct] if ct is not None else 0)) / (xc.pow(2).mean() + o.cfg.eps).sqrt()
    src, heads, terms = [], [], []
    for l in range(nl):
        b = o.w["blocks"][l]
        x = o._ln_pre(cache[f"blocks.{l}.hook_resid_pre"])
        qq = torch.einsum("bpd,hde->bphe", x, b["W_Q"]) + b["b_Q"]
        kk = torch.einsum("bpd,hde->bphe", x, b["W_K"]) + b["b_K"]
        vv = torch.einsum("bpd,hde->bphe", x, b["W_V"]) + b["b_V"]
        sc = torch.einsum("bqhe,bkhe->bhqk", o._rotate(qq), o._rotate(kk)) / math.sqrt(DH)
        p = torch.softmax(sc[0, :, q, :q + 1], dim=-1)                 # [H][q + 1]
        r = torch.einsum("jhe,hed->hjd", vv[0, :q + 1], b["W_O"])       # [H][q + 1][d]
        src.append(p * (r @ dirs))
        terms.append(p * (r.abs() @ dirs.abs()))
        heads.append(cache[f"blocks.{l}.attn.hook_result"][0, q] @ dirs)
    f = lambda ts: torch.stack(ts).double().numpy()  # noqa: E731
    return f(src), f(heads), f(terms)


_oracle_cache = {}


def oracle_pair(cfg, sd, tok):
    if "pair" not in _oracle_cache:
        pair = []
        for dt in (torch.float32, torch.float64):
            o = make_oracle(cfg, sd, tok, dt)
            o.cfg.use_attn_result = True  # (this module's own oracles: hook_result is cached)
            pair.append(o)
        _oracle_cache["pair"] = pair
    return _oracle_cache["pair"]


def oracle_data(cfg, sd, tok, key, seqs, qpos, tg, ct):
    """Per prompt (src64, heads64) and the bars (src, the sum over keys of src, heads), from the two oracles alone:
    computed once per key for the module."""
    if key not in _oracle_cache:
        o32, o64 = oracle_pair(cfg, sd, tok)
        data, e_src, e_sum, e_heads, t_max = [], 0.0, 0.0, 0.0, 0.0
        for s, (ids, q) in enumerate(zip(seqs, qpos)):
            a32 = oracle_sources(o32, ids, q, tg[s], None if ct is None else ct[s])
            a64 = oracle_sources(o64, ids, q, tg[s], None if ct is None else ct[s])
            assert np.abs(a64[0].sum(-1) - a64[1]).max() <= 1e-12 * max(1.0, a64[2].sum(-1).max())  # (b_V = 0)
            e_src = max(e_src, np.abs(a32[0] - a64[0]).max())
            e_sum = max(e_sum, np.abs(a32[0].sum(-1) - a64[0].sum(-1)).max())
            e_heads = max(e_heads, np.abs(a32[1] - a64[1]).max())
            t_max = max(t_max, a64[2].sum(-1).max())  # (a head's sum of |terms|: the floor of the summed quantities)
            data.append((a64[0], a64[1], a64[2]))
        f_src = 4.0 * EPS24 * max(d[2].max() for d in data)
        f_sum = 4.0 * EPS24 * t_max
        _oracle_cache[key] = (data, dict(src=max(4.0 * e_src, f_src), sum=max(4.0 * e_sum, f_sum),
                                         heads=max(4.0 * e_heads, f_sum)))
    return _oracle_cache[key]


@pytest.mark.parametrize("pos_key", (None, "mid"))
@pytest.mark.parametrize("ct_key", (None, "contrast"))
def test_end_to_end_against_the_oracle(tiny_model, tiny_cfg, tiny_sd, tokenizer, pos_key, ct_key):
    seqs = ragged_prompts(tiny_cfg, LENS)
    pos = None if pos_key is None else list(MID)
    qpos = [len(s) - 1 for s in seqs] if pos is None else pos
    ct = None if ct_key is None else list(CONTRAST)
    data, bars = oracle_data(tiny_cfg, tiny_sd, tokenizer, (pos_key, ct_key), seqs, qpos, list(TARGETS), ct)
    trace = filled_trace(tiny_model, seqs)
    src = trace.source_attribution(list(TARGETS), contrast=ct, pos=pos, want_keys=True)[0].double().cpu().numpy()
    heads = trace.logit_attribution(list(TARGETS), contrast=ct, pos=pos)[0].double().cpu().numpy()
    g = tiny_model.gemm
    e_src = max(np.abs(src[s, :, :, :q + 1] - data[s][0]).max() for s, q in enumerate(qpos))
    e_cons = max(np.abs(src[s].sum(-1) - heads[s]).max() for s in range(len(seqs)))
    print(f"source attribution vs fp64 oracle ({g}, pos {pos_key}, contrast {ct_key}): src {e_src:.3e} / {bars['src']:.3e}, "
          f"sum over keys vs out_head {e_cons:.3e} / {bars['sum'] + bars['heads']:.3e}")
    ok = note(f"oracle end to end src {g}", e_src, bars["src"])
    ok_c = note(f"conservation vs out_head {g}", e_cons, bars["sum"] + bars["heads"])
    assert ok and ok_c, (e_src, e_cons, bars)


# ------------------------------------------------------------------------------ 5: the façade
PROFILE_SEED, N_CONTEXTS, LEN_CONTEXTS, TOP_N = 3, 8, 2, 2


def test_head_source_attribution_against_the_oracle(tiny_model, tiny_cfg, tiny_sd, tokenizer):
    cfg, g = tiny_cfg, tiny_model.gemm
    contexts = list(tvr_amd.tasks.letter_to_caps)
    random.seed(PROFILE_SEED)
    seqs, roles, answers = experiments.knockout_role_prompts(tiny_model, contexts, ARROW, ",", N_CONTEXTS, LEN_CONTEXTS)
    random.seed(PROFILE_SEED)
    prof = experiments.head_source_attribution(contexts, ARROW, ",", model=tiny_model, num_contexts=N_CONTEXTS,
                                               len_contexts=LEN_CONTEXTS)
    assert tuple(prof.shape) == (cfg.n_layers, cfg.n_heads, len(ROLES))
    if "facade" not in _oracle_cache:
        o32, o64 = oracle_pair(cfg, tiny_sd, tokenizer)
        by = {}
        for name, o in (("32", o32), ("64", o64)):
            out = np.zeros((len(seqs), cfg.n_layers, cfg.n_heads, len(ROLES)))
            heads = np.zeros((len(seqs), cfg.n_layers, cfg.n_heads))
            terms = 0.0
            for s, (ids, r) in enumerate(zip(seqs, roles)):
                a = oracle_sources(o, ids, len(ids) - 1, answers[s], None)
                r = np.asarray(r)
                for c in range(len(ROLES)):
                    out[s, :, :, c] = a[0][:, :, r == c].sum(-1)
                heads[s] = a[1]
                terms = max(terms, a[2].sum(-1).max())
            by[name] = (out, heads, terms)
        _oracle_cache["facade"] = by
    by = _oracle_cache["facade"]
    floor = 4.0 * EPS24 * by["64"][2]
    bar = max(4.0 * np.abs(by["32"][0] - by["64"][0]).max(), floor)
    bar_h = max(4.0 * np.abs(by["32"][1] - by["64"][1]).max(), floor)
    ref = by["64"][0].mean(0)
    got = prof.double().cpu().numpy()
    err = np.abs(got - ref).max()  # a mean over prompts: at most the largest error of its terms
    print(f"head_source_attribution ({g}): err {err:.3e}, bar {bar:.3e}")
    assert note(f"facade head_source_attribution {g}", err, bar)
    # its sum over the roles is head_logit_attribution(...).heads on the same prompts: both held to the oracle
    heads = experiments.head_logit_attribution(seqs, answers, model=tiny_model).heads.double().cpu().numpy()
    assert note(f"facade sum over roles vs heads {g}", np.abs(got.sum(-1) - heads).max(), bar + bar_h)
    # the selection: the oracle's top heads, where the oracle separates rank n from rank n + 1
    role = ROLES.index("demo_label")
    order = np.sort(ref[:, :, role].ravel())[::-1]
    assert order[TOP_N - 1] - order[TOP_N] > 2 * bar, "choose another PROFILE_SEED: the reference has no gap"
    want = {(int(i) // cfg.n_heads, int(i) % cfg.n_heads) for i in np.argsort(-ref[:, :, role].ravel())[:TOP_N]}
    assert set(experiments.top_source_heads(prof, "demo_label", TOP_N)) == want
    # with contrast answers: the same call on the differences (engine-internal: against Trace.source_attribution)
    contrast = [[CONTRAST[0]]] * len(seqs)
    random.seed(PROFILE_SEED)
    prof_c = experiments.head_source_attribution(contexts, ARROW, ",", model=tiny_model, num_contexts=N_CONTEXTS,
                                                 len_contexts=LEN_CONTEXTS, contrast_answers=contrast)
    trace = filled_trace(tiny_model, seqs)
    by_c = trace.source_attribution(answers, contrast=[CONTRAST[0]] * len(seqs), classes=roles, n_classes=len(ROLES))[1]
    assert (bits((by_c.sum(0) / len(seqs)).cpu().numpy()) == bits(prof_c.cpu().numpy())).all()
