"""Direct logit attribution and the logit lens on the GPU: ``head_attribution_kernel``
alone (``tvr_head_attribution``), on a trace (``tvr_trace_logit_attribution``),
the lens and the decoder over the engine's final stage (``tvr_trace_logit_lens``,
``tvr_decode_rows``) and the façade, against the fp64 references of
tests/attribution_cases.py and the fp64 oracle.

Primitive: one small two-layer model per (d_head, n_heads) of
attention_cases.MODELS, its layer-1 W_O the operand.  Every launch (``run``)
writes into a NaN-filled buffer at an offset that is only 4-byte aligned and
checks, bit for bit, that nothing outside [n][H] is written; z and dirs carry
NaN rows beyond n, which must not reach any output.  Bars
(attribution_cases.bar): 4 x the larger error of two fp32 restatements, floored
at 4 x 2^-24 x the largest sum of |terms|.  ``select`` is bit-exact, ``zero`` rows
are exactly 0, a second run gives identical bits, and each row computed alone
(n = 1) has the bits it has inside n = 33.

Trace path: heads and resid against the fp64 reference built from the trace's OWN
exported hook_z / hook_resid_pre rows and the model's fp32 weights, at the bars
of the same two restatements, on the three GEMM paths and on an exact-fp16 model
(uncentred trace); a pending (deferred) trace gives the bits of a filled one.

End to end against the fp64 oracle: heads, embed and total at
max(4 x |fp32 oracle - fp64 oracle|, floor) (the margin-of-4 convention of
test_gpu_attention_pattern.py; floor 4 x 2^-24 x the largest sum of |terms| of
the total), ``rest`` (resid[l + 1] - resid[l] - the sum of the heads, from the
engine's fp32 outputs) at the same bar from the oracles' own rest
(hook_attn_out - the sum of hook_result + hook_mlp_out).  Conservation on the engine:
resid[:, L] + the b_U difference against Model.forward's logit difference at the
resid bar.

Lens and decode: row L of the lens against forward_clean's probability at the
project's 1e-4-of-the-maximum bar; the lens equals ``decode_rows`` of the same
rows in the same order BIT FOR BIT on a centred trace (same rows, same launch
shape, hence the same GEMM plan); decoded layer by layer (another launch shape,
possibly another plan) and on the exact-fp16 model (whose export is re-centred:
other input bits) it agrees at the 1e-4 bar.  Every layer's probability against
the fp64 oracle at max(4 x |fp32 oracle - fp64 oracle|, 2^-22); top-k ids as sets
on the rows where the fp64 logit gap between ranks k and k + 1 exceeds the logit
bar, at most 10 % of the rows skipped (asserted; none is with these prompts), and
in order (descending) on the rows where every gap between ranks 1 .. k + 1 does.
``decode_rows`` of more rows than one chunk of the final stage (1,061 on the f32
path, whose chunk is 1,024) against fp64, against launches of one chunk each and
against single rows across the chunk edge.

Measured on an MI355X by this file (worst err / bar, printed at its end).
Primitive, worst over the five kinds, n = 1 / 15 / 16 / 17 / 33:
  d_head  16: 0.073 0.148 0.108 0.069 0.128
  d_head  64: 0.013 0.049 0.034 0.034 0.025
  d_head  80: 0.039 0.028 0.021 0.039 0.031
  d_head 128: 0.038 0.026 0.037 0.027 0.020
(the bar is its floor of 4 ulps of the sum of |terms| in most cases: the MFMA's
fma chains over d / 4 rows per wave, summed over four waves and four z chains,
stay an order of magnitude below it); select bitwise at every d_head.  Trace
against its own rows, heads / resid: f32 0.054 / 0.081, x2f16 0.043 / 0.068,
x3bf16 0.068 / 0.145, exact-fp16 0.047 / 0.187.  End to end against the fp64
oracle (bars 1.4e-6 .. 3.9e-6; the margin of 4 holds), heads / rest / embed /
total: f32 0.181 / 0.381 / 0.010 / 0.501, x2f16 0.148 / 0.268 / 0.011 / 0.379,
x3bf16 0.135 / 0.512 / 0.010 / 0.379.  The two figures at 0.5 were examined: the
total is one residual row, and rest a difference of two, that the CLEAN FORWARD
computed (its GEMMs' error against the fp64 oracle, the same rows the oracle
parity tests bound); against the trace's own rows the attribution kernels stay
below 0.19 of bars of the same size, so no summation order of theirs is behind it.  Conservation against Model.forward: f32
0.187, x2f16 0.076, x3bf16 0.111.  Lens probability against the oracle at most
0.013 of its bar, row L against forward_clean at most 0.002 of the 1e-4 bar,
the lens against decode_rows layer by layer 0.000 (identical to the digits
printed) and bit for bit in one launch.  decode_rows of 1,061 rows 0.006 of the
1e-4 bar.  Façade: heads at most 0.034, rest 0.051, total 0.026.  The whole file
(55 tests) runs in about 2 s.
"""
import collections
import functools
import gc
import time

import numpy as np
import pytest
import torch

import attention_cases as A
import attribution_cases as C
import tvr_amd
from conftest import make_oracle
from tvr_amd import _lib as L, experiments

pytestmark = [pytest.mark.gpu]

G = 3                  # guard rows (of H floats) before and after every output
NAN_BITS = 0x7FC00000  # torch.full(nan)
FP32_TOL = 1e-4        # the project's bar on a probability: 1e-4 of the maximum (tests/test_gpu_engine.py)
MODEL_IDS = [f"dh{dh}h{h}" for dh, h in A.MODELS]
LENS = (7, 12, 5, 9)
MID = (3, 0, 4, 8)
TARGETS = (5, 77, 300, 41)
CONTRAST = (9, 3, 411, 200)
TOPK = 3

_worst = collections.defaultdict(float)


def note(form, err, bar):
    _worst[form] = max(_worst[form], err / bar)
    return err <= bar


@pytest.fixture(scope="module", autouse=True)
def _module():
    t0 = time.time()
    yield
    for form, r in sorted(_worst.items()):
        print(f"\nlogit attribution, worst err / bar: {form:44s} {r:.3f}", end="")
    print(f"\nlogit attribution tests: {time.time() - t0:.1f} s from the first test to the last")
    _ctx.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


class Ctx:
    def __init__(self, DH, H):
        self.DH, self.H, self.d = DH, H, DH * H
        cfg = tvr_amd.config.PythiaConfig(2, self.d, H, C.D_MLP, 64, n_ctx=64, name=f"attribution-{DH}x{H}")
        w = tvr_amd.weights.synth_engine_weights(cfg, seed=1, device="cuda", std=0.2)
        self.model = tvr_amd.Model(cfg, w, tokenizer=tvr_amd.tokenizer.SyntheticTokenizer(512), device="cuda", gemm="f32")
        self.lib, self.h = self.model._lib, self.model._h
        self.W = [lay.w2.cpu().numpy() for lay in w.layers]

    def stream(self):
        return self.model._stream()


@functools.lru_cache(maxsize=None)  # one model per (d_head, n_heads) for the module: _module clears it
def _ctx(model):
    return Ctx(*model)


@pytest.fixture(params=A.MODELS, ids=MODEL_IDS)
def ctx(request):
    return _ctx(request.param)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def nan_padded(a, extra=2):
    """a [n][d] on the device with ``extra`` NaN rows behind it (16-byte aligned: a fresh allocation)."""
    t = torch.full((a.shape[0] + extra, a.shape[1]), float("nan"), dtype=torch.float32, device="cuda")
    t[:a.shape[0]] = torch.from_numpy(a)
    return t


class Guarded:
    """A NaN-filled float buffer with [n][H] inside it, G rows of guard on either side, starting ``shift``
    floats into the allocation (shift = 1: 4-byte aligned only)."""

    def __init__(self, n, H, shift=1):
        self.n, self.H, self.shift = n, H, shift
        self.t = torch.full(((n + 2 * G) * H + 4,), float("nan"), dtype=torch.float32, device="cuda")
        self.at = shift + G * H
        self.ptr = self.t.data_ptr() + 4 * self.at

    def read(self, what):
        h = self.t.cpu().numpy()
        b = h.view(np.int32)
        inside = np.zeros(h.shape, dtype=bool)
        inside[self.at:self.at + self.n * self.H] = True
        assert (b[~inside] == NAN_BITS).all(), f"{what}: written outside [n][H]"
        return h[inside].reshape(self.n, self.H).copy()

    def untouched(self):
        return (self.t.cpu().numpy().view(np.int32) == NAN_BITS).all()


def run(ctx, case, layer=1, shift=1, n=None):
    """One tvr_head_attribution launch of the case's first n rows: out [n][H]."""
    if not hasattr(case, "dev"):
        case.dev = (nan_padded(case.z), nan_padded(case.dirs))
    n = case.n if n is None else n
    out = Guarded(n, ctx.H, shift)
    assert shift == 0 or out.ptr % 16 != 0  # (4-byte aligned only)
    rc = ctx.lib.tvr_head_attribution(ctx.h, layer, case.dev[0].data_ptr(), case.dev[1].data_ptr(), n, out.ptr, ctx.stream())
    L.check(rc, "tvr_head_attribution")
    got = out.read("out")
    assert not np.isnan(got).any(), "NaN in the output: a row beyond n was read"
    return got


# ------------------------------------------------------------------------------ 1: the primitive
def test_primitive_against_fp64(ctx):
    model = (ctx.DH, ctx.H)
    for n in C.ALL_N:
        for kind in C.KINDS:
            case = C.make(kind, ctx.DH, ctx.H, n, W=ctx.W[1])
            ref = C.reference(case)
            bar = C.bar(case, ref)[0]
            got = run(ctx, case, shift=1 if n != 16 else 0)
            err = C.max_err(got, ref)
            ok = note(f"primitive d_head {ctx.DH:3d} n {n:2d}", err, bar)
            print(f"head attribution {model} {kind:7s} n {n:2d}: err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
            assert ok, (model, kind, n, err, bar)
            assert (bits(run(ctx, case)) == bits(got)).all(), "a second run gives other bits"
            if kind == "select":
                assert (bits(got) == bits(case.exact)).all(), (model, n)
            if kind == "zero":
                assert (got[C.zero_rows(case)] == 0).all()


def test_layer_selects_its_own_weights(ctx):
    case = C.make("random", ctx.DH, ctx.H, 17, W=ctx.W[0], seed=3)
    ref = C.reference(case)
    err, bar = C.max_err(run(ctx, case, layer=0), ref), C.bar(case, ref)[0]
    assert note(f"primitive d_head {ctx.DH:3d} layer 0", err, bar)
    assert C.max_err(run(ctx, case, layer=1), ref) > 100 * bar  # (the other layer's W_O is another matrix)


def test_a_row_alone_has_the_bits_it_has_in_a_batch(ctx):
    for kind in ("random", "gain"):
        case = C.make(kind, ctx.DH, ctx.H, 33, W=ctx.W[1])
        full = run(ctx, case)
        for n in (1, 16, 17):  # a prefix of the rows: another chunk count, another last-chunk mask
            assert (bits(run(ctx, case, n=n)) == bits(full[:n])).all(), (kind, n)
        for i in range(33):
            one = C.Case(kind, ctx.DH, ctx.H, case.W, case.z[i:i + 1].copy(), case.dirs[i:i + 1].copy())
            assert (bits(run(ctx, one, shift=i % 2)) == bits(full[i:i + 1])).all(), (kind, i)


# ------------------------------------------------------------------------------ 2: errors
def test_invalid_primitive_arguments_launch_nothing():
    ctx = _ctx(A.MODELS[0])
    case = C.make("random", ctx.DH, ctx.H, 17, W=ctx.W[1])
    ref = run(ctx, case)
    z, dirs = case.dev[0].data_ptr(), case.dev[1].data_ptr()
    out = Guarded(17, ctx.H)

    def refused(message, layer, zp, dp, n, op, model=ctx.h):
        rc = ctx.lib.tvr_head_attribution(model, layer, zp, dp, n, op, ctx.stream())
        err = ctx.lib.tvr_last_error().decode()
        assert rc == L.TVR_ERR_INVALID and err.startswith("tvr_head_attribution: ") and message in err, (message, rc, err)

    refused("null model", 1, z, dirs, 17, out.ptr, model=None)
    refused("null argument", 1, None, dirs, 17, out.ptr)
    refused("null argument", 1, z, None, 17, out.ptr)
    refused("null argument", 1, z, dirs, 17, None)
    refused("n must be positive", 1, z, dirs, 0, out.ptr)
    refused("n must be positive", 1, z, dirs, -3, out.ptr)
    refused("layer out of range", -1, z, dirs, 17, out.ptr)
    refused("layer out of range", 2, z, dirs, 17, out.ptr)
    refused("16-byte aligned", 1, z + 4, dirs, 16, out.ptr)
    refused("16-byte aligned", 1, z, dirs + 8, 16, out.ptr)
    torch.cuda.synchronize()
    assert out.untouched()
    L.check(ctx.lib.tvr_head_attribution(ctx.h, 1, z, dirs, 17, out.ptr, ctx.stream()), "tvr_head_attribution")
    assert (bits(out.read("out")) == bits(ref)).all()  # the model is still usable


def ragged_prompts(cfg, lens, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [[0] + torch.randint(1, cfg.d_vocab, (n - 1,), generator=g).tolist() for n in lens]


def filled_trace(model, prompts, defer=False):
    trace = model.trace(len(prompts), sum(map(len, prompts)))
    model.forward_clean(prompts, trace=trace, defer=defer)
    return trace


def i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def p(a):
    return None if a is None else a.ctypes.data


def test_invalid_trace_and_decode_arguments_launch_nothing(tiny_model):
    cfg, lib, st = tiny_model.cfg, tiny_model._lib, tiny_model._stream()
    seqs = ragged_prompts(cfg, LENS)
    n, nl, H, V, d = len(seqs), cfg.n_layers, cfg.n_heads, cfg.d_vocab, cfg.d_model
    empty = tiny_model.trace(n, sum(LENS))
    trace = filled_trace(tiny_model, seqs)
    heads, resid = Guarded(n * nl, H), Guarded(n, nl + 1)
    prob = Guarded(n, nl + 1)
    top = torch.full((n, nl + 1, TOPK), -7, dtype=torch.int32, device="cuda")
    tg, ct = i32(TARGETS), i32(CONTRAST)

    def refused(fn, message, *args):
        rc = getattr(lib, fn)(*args, st)
        err = lib.tvr_last_error().decode()
        assert rc == L.TVR_ERR_INVALID and err.startswith(fn + ": ") and message in err, (fn, message, rc, err)

    def att(message, tr, pos, t, c, hp, rp):
        refused("tvr_trace_logit_attribution", message, tr._h, p(i32(pos)), p(i32(t)), p(i32(c)), hp, rp)

    att("null target", trace, None, None, ct, heads.ptr, resid.ptr)
    att("both null", trace, None, tg, ct, None, None)
    att("trace is empty", empty, None, tg, ct, heads.ptr, resid.ptr)
    att("pos of sequence 1 out of range", trace, [0, 12, 0, 0], tg, ct, heads.ptr, resid.ptr)
    att("pos of sequence 0 out of range", trace, [-1, 0, 0, 0], tg, ct, heads.ptr, resid.ptr)
    att("target of sequence 2 outside", trace, None, [1, 2, V, 3], ct, heads.ptr, resid.ptr)
    att("target of sequence 0 outside", trace, None, [-1, 2, 3, 3], None, heads.ptr, resid.ptr)
    att("contrast of sequence 3 outside", trace, None, tg, [1, 2, 3, V], heads.ptr, resid.ptr)
    att("contrast of sequence 1 outside", trace, None, tg, [1, -2, 3, 4], heads.ptr, None)

    def lens(message, tr, pos, t, pp, kp, k):
        refused("tvr_trace_logit_lens", message, tr._h, p(i32(pos)), p(i32(t)), pp, kp, k)

    lens("trace is empty", empty, None, tg, prob.ptr, top.data_ptr(), TOPK)
    lens("both null", trace, None, tg, None, None, TOPK)
    lens("out_prob needs targets", trace, None, None, prob.ptr, top.data_ptr(), TOPK)
    lens("topk must be in [1, 16] with out_topk", trace, None, tg, prob.ptr, top.data_ptr(), 0)
    lens("topk must be in [1, 16] with out_topk", trace, None, tg, None, top.data_ptr(), 17)
    lens("topk must be in [0, 16]", trace, None, tg, prob.ptr, None, -1)
    lens("topk must be in [0, 16]", trace, None, tg, prob.ptr, None, 17)
    lens("pos of sequence 2 out of range", trace, [0, 0, 5, 0], tg, prob.ptr, None, 0)
    lens("target 1 outside", trace, None, [1, V, 2, 3], prob.ptr, None, 0)

    rows = torch.randn(n + 1, d, device="cuda")
    dprob = Guarded(n, 1)

    def dec(message, rp, nn, t, pp, kp, k, model=tiny_model._h):
        refused("tvr_decode_rows", message, model, rp, nn, p(i32(t)), pp, kp, k)

    dec("null model", rows.data_ptr(), n, tg, dprob.ptr, None, 0, model=None)
    dec("null rows", None, n, tg, dprob.ptr, None, 0)
    dec("n must be positive", rows.data_ptr(), 0, tg, dprob.ptr, None, 0)
    dec("16-byte aligned", rows.data_ptr() + 4, n, tg, dprob.ptr, None, 0)
    dec("both null", rows.data_ptr(), n, tg, None, None, 1)
    dec("out_prob needs targets", rows.data_ptr(), n, None, dprob.ptr, None, 0)
    dec("topk must be in [1, 16] with out_topk", rows.data_ptr(), n, None, None, top.data_ptr(), 0)
    dec("topk must be in [1, 16] with out_topk", rows.data_ptr(), n, None, None, top.data_ptr(), 17)
    dec("target 3 outside", rows.data_ptr(), n, [1, 2, 3, -1], dprob.ptr, None, 0)
    torch.cuda.synchronize()
    assert heads.untouched() and resid.untouched() and prob.untouched() and dprob.untouched()
    assert (top == -7).all().item()
    # the façade's own checks come first and raise ValueError as well
    with pytest.raises(ValueError, match="outside its sequence"):
        trace.logit_attribution(list(TARGETS), pos=[0, 12, 0, 0])
    with pytest.raises(ValueError, match="trace is empty"):
        empty.logit_lens(list(TARGETS))
    # afterwards the trace and the model are still usable: valid calls on the same buffers, offset outputs
    L.check(lib.tvr_trace_logit_attribution(trace._h, None, p(tg), p(ct), heads.ptr, resid.ptr, st), "attribution")
    h, r = trace.logit_attribution(list(TARGETS), contrast=list(CONTRAST))
    assert (bits(heads.read("out_head")) == bits(h.cpu().numpy().reshape(n * nl, H))).all()
    assert (bits(resid.read("out_resid")) == bits(r.cpu().numpy())).all()
    L.check(lib.tvr_trace_logit_lens(trace._h, None, p(tg), prob.ptr, None, 0, st), "lens")  # topk ignored without out_topk
    assert (bits(prob.read("out_prob")) == bits(trace.logit_lens(list(TARGETS))[0].cpu().numpy())).all()
    # one output alone is enough
    only_h = Guarded(n * nl, H)
    L.check(lib.tvr_trace_logit_attribution(trace._h, None, p(tg), p(ct), only_h.ptr, None, st), "attribution")
    assert (bits(only_h.read("out_head")) == bits(heads.read("out_head"))).all()


# ------------------------------------------------------------------------------ 3: the trace path
@pytest.fixture(scope="module")
def exact16_model(tiny_cfg, tokenizer):
    """fp16-valued weights: the exact-fp16 GEMMs are bound and the trace is uncentred (as
    tests/test_gpu_task_vectors.py builds its model)."""
    sd = tvr_amd.weights.synth_hf_state_dict(tiny_cfg, seed=0, std=0.3, fp16=True)
    m = tvr_amd.Model.from_hf_state_dict(tiny_cfg, sd, device="cuda", tokenizer=tokenizer, gemm="x2f16")
    assert m.exact16
    return m


def trace_arrays(model, trace, qpos):
    """x [L + 1][n][d], z [L][n][d] (the trace's own exported rows at the query positions), Ws, W_U' rows."""
    nl = model.cfg.n_layers
    rows = torch.as_tensor([o + q for o, q in zip(trace.seq_offsets, qpos)], device=model.device)
    x = np.stack([trace.resid_pre(l)[rows].cpu().numpy() for l in range(nl + 1)])
    z = np.stack([trace.z(l)[rows].cpu().numpy() for l in range(nl)])
    Ws = [lay.w2.cpu().numpy() for lay in model.weights.layers]
    return x, z, Ws, model.weights.w_unembed_t.cpu().numpy()


def check_trace_path(model, name):
    cfg = model.cfg
    seqs = ragged_prompts(cfg, LENS)
    trace = filled_trace(model, seqs)
    pending = filled_trace(model, seqs, defer=True)
    first = True
    for pos in (None, MID):
        qpos = [len(s) - 1 for s in seqs] if pos is None else list(pos)
        x, z, Ws, wu = trace_arrays(model, trace, qpos)
        for ct in (None, CONTRAST):
            ut, uc = wu[list(TARGETS)], (None if ct is None else wu[list(ct)])
            ref = C.attribution(x, z, Ws, ut, uc, cfg.ln_eps, cfg.d_model // cfg.n_heads)
            bars = C.attribution_bar(x, z, Ws, ut, uc, cfg.ln_eps, cfg.d_model // cfg.n_heads, ref)
            heads, resid = trace.logit_attribution(list(TARGETS), contrast=ct, pos=pos)
            eh, er = C.max_err(heads.cpu().numpy(), ref[0]), C.max_err(resid.cpu().numpy(), ref[1])
            print(f"trace attribution ({name}, pos {pos}, contrast {ct is not None}): heads {eh:.3e} / {bars[0]:.3e}, "
                  f"resid {er:.3e} / {bars[1]:.3e}")
            ok_h, ok_r = note(f"trace heads vs own rows {name}", eh, bars[0]), note(f"trace resid vs own rows {name}", er, bars[1])
            assert ok_h and ok_r, (name, pos, ct, eh, er, bars)
            if first:  # the deferred clean forward runs inside the call: the same bits as on the filled trace
                h2, r2 = pending.logit_attribution(list(TARGETS), contrast=ct, pos=pos)
                assert (bits(h2.cpu().numpy()) == bits(heads.cpu().numpy())).all()
                assert (bits(r2.cpu().numpy()) == bits(resid.cpu().numpy())).all()
                first = False
            h3, r3 = model.logit_attribution(trace, list(TARGETS), contrast=ct, positions=pos)
            assert (bits(h3.cpu().numpy()) == bits(heads.cpu().numpy())).all()  # reproducible


def test_trace_path_against_its_own_rows(tiny_model):
    check_trace_path(tiny_model, tiny_model.gemm)


def test_trace_path_on_an_uncentred_trace(exact16_model):
    check_trace_path(exact16_model, "exact-fp16")


def test_trace_head_pass_is_the_primitive(tiny_model):
    """One kernel, two callers: the primitive on the exported z rows and the trace path's own directions
    (recovered as resid's operand is not exported: dirs = u / sigma in fp32, as the kernel forms it)."""
    cfg = tiny_model.cfg
    seqs = ragged_prompts(cfg, LENS)
    trace = filled_trace(tiny_model, seqs)
    heads, _ = trace.logit_attribution(list(TARGETS))
    rows = torch.as_tensor([o + n - 1 for o, n in zip(trace.seq_offsets, LENS)], device="cuda")
    xL = trace.resid_pre(cfg.n_layers)[rows]
    xc = xL - xL.mean(-1, keepdim=True)
    sigma = (xc.pow(2).mean(-1, keepdim=True) + cfg.ln_eps).sqrt()
    dirs = tiny_model.weights.w_unembed_t[list(TARGETS)] / sigma
    for l in range(cfg.n_layers):
        got = tiny_model.head_attribution(l, trace.z(l)[rows], dirs)
        # torch's mean / sqrt may differ from the kernel's by an ulp of sigma: 2^-22 relative to the sum of |terms|
        terms = C.heads_terms(trace.z(l)[rows].cpu().numpy(), dirs.cpu().numpy(), tiny_model.weights.layers[l].w2.cpu().numpy(),
                              cfg.d_model // cfg.n_heads)
        assert (np.abs(got.cpu().numpy().astype(np.float64) - heads[:, l].cpu().numpy()) <= 2.0 ** -21 * terms).all()


# ------------------------------------------------------------------------------ 4 - 6: against the oracle
def oracle_pair(cfg, sd, tok):
    out = []
    for dt in (torch.float32, torch.float64):
        o = make_oracle(cfg, sd, tok, dt)
        o.cfg.use_attn_result = True  # (this module's own oracles: hook_result is cached)
        out.append(o)
    return out


def oracle_quantities(o, seqs, qpos, tg, ct):
    """fp64 arrays computed in the oracle's dtype: heads [n][L][H], rest [n][L], resid [n][L + 1], the logit
    difference minus b_U's [n], the lens logits [n][L + 1][V], sum of |terms| of the total [n]."""
    nl = o.cfg.n_layers
    WU, bU = o.w["W_U"], o.w["b_U"]
    heads, rest, resid, diff, lens, terms = [], [], [], [], [], []
    for s, (ids, q) in enumerate(zip(seqs, qpos)):
        logits, cache = o.run_with_cache(torch.tensor([ids]))
        xs = [cache[f"blocks.{l}.hook_resid_pre"][0, q] for l in range(nl)] + [cache[f"blocks.{nl - 1}.hook_resid_post"][0, q]]
        xc = xs[nl] - xs[nl].mean()
        sigma = (xc.pow(2).mean() + o.cfg.eps).sqrt()
        u = WU[:, tg[s]] - (WU[:, ct[s]] if ct is not None else 0)
        dirs = u / sigma
        heads.append(torch.stack([cache[f"blocks.{l}.attn.hook_result"][0, q] @ dirs for l in range(nl)]))
        rest.append(torch.stack([((cache[f"blocks.{l}.hook_attn_out"][0, q] - cache[f"blocks.{l}.attn.hook_result"][0, q].sum(0))
                                  + cache[f"blocks.{l}.hook_mlp_out"][0, q]) @ dirs for l in range(nl)]))
        resid.append(torch.stack([(x - x.mean()) @ dirs for x in xs]))
        dl = logits[0, q, tg[s]] - bU[tg[s]]
        if ct is not None:
            dl = dl - (logits[0, q, ct[s]] - bU[ct[s]])
        diff.append(dl)
        lens.append(torch.stack([o._ln_pre(x) @ WU + bU for x in xs]))
        terms.append((xc.abs() * dirs.abs()).sum())
    f = lambda ts: torch.stack(ts).double().numpy()  # noqa: E731
    return f(heads), f(rest), f(resid), f(diff), f(lens), f(terms)


_oracle_cache = {}


def oracle_data(cfg, sd, tok, pos_key, ct_key):
    """(fp64 quantities, bars) for LENS at pos None / MID, contrast None / CONTRAST: computed once for the module."""
    key = (pos_key, ct_key)
    if key not in _oracle_cache:
        if "pair" not in _oracle_cache:
            _oracle_cache["pair"] = oracle_pair(cfg, sd, tok)
        o32, o64 = _oracle_cache["pair"]
        seqs = ragged_prompts(cfg, LENS)
        qpos = [len(s) - 1 for s in seqs] if pos_key is None else list(MID)
        ct = None if ct_key is None else list(CONTRAST)
        q32 = oracle_quantities(o32, seqs, qpos, list(TARGETS), ct)
        q64 = oracle_quantities(o64, seqs, qpos, list(TARGETS), ct)
        floor = C.floor_of(q64[5])
        bar_h = max(4.0 * np.abs(q32[0] - q64[0]).max(), floor)
        bar_r = max(4.0 * np.abs(q32[2] - q64[2]).max(), floor)
        bar_rest = max(4.0 * np.abs(q32[1] - q64[1]).max(), floor)
        bar_logit = max(4.0 * np.abs(q32[4] - q64[4]).max(), 2.0 ** -22 * np.abs(q64[4]).max())
        p32, p64 = torch.softmax(torch.from_numpy(q32[4]), -1).numpy(), torch.softmax(torch.from_numpy(q64[4]), -1).numpy()
        bar_p = max(4.0 * np.abs(p32 - p64).max(), 2.0 ** -22)
        _oracle_cache[key] = (q64, p64, dict(heads=bar_h, resid=bar_r, rest=bar_rest,
                                             logit=bar_logit, prob=bar_p))
    return _oracle_cache[key]


def ordered_topk_rows(logits64, k, bar):
    """Rows whose fp64 gaps between ALL neighbouring ranks 1 .. k + 1 exceed the bar: there the top-k ids are
    determined in order (descending)."""
    srt = np.sort(logits64, -1)[..., ::-1]
    return ((srt[..., :k] - srt[..., 1:k + 1]) > bar).all(-1)


def robust_topk_rows(logits64, k, bar):
    """Rows whose fp64 gap between ranks k and k + 1 exceeds the bar, and the fp64 top-k ids (descending)."""
    srt = np.sort(logits64, -1)[..., ::-1]
    keep = (srt[..., k - 1] - srt[..., k]) > bar
    ids = np.argsort(-logits64, -1)[..., :k]
    return keep, ids


@pytest.mark.parametrize("pos_key", (None, "mid"))
@pytest.mark.parametrize("ct_key", (None, "contrast"))
def test_end_to_end_against_the_oracle(tiny_model, tiny_cfg, tiny_sd, tokenizer, pos_key, ct_key):
    q64, _, bars = oracle_data(tiny_cfg, tiny_sd, tokenizer, pos_key, ct_key)
    seqs = ragged_prompts(tiny_cfg, LENS)
    pos = None if pos_key is None else list(MID)
    ct = None if ct_key is None else list(CONTRAST)
    trace = filled_trace(tiny_model, seqs)
    heads, resid = trace.logit_attribution(list(TARGETS), contrast=ct, pos=pos)
    heads, resid = heads.double().cpu().numpy(), resid.double().cpu().numpy()
    rest = resid[:, 1:] - resid[:, :-1] - heads.sum(-1)
    g = tiny_model.gemm
    errs = dict(heads=np.abs(heads - q64[0]).max(), rest=np.abs(rest - q64[1]).max(),
                embed=np.abs(resid[:, 0] - q64[2][:, 0]).max(), total=np.abs(resid[:, -1] - q64[2][:, -1]).max(),
                resid=np.abs(resid - q64[2]).max())
    print(f"attribution vs fp64 oracle ({g}, pos {pos_key}, contrast {ct_key}): " +
          ", ".join(f"{k} {e:.3e} / {bars['resid' if k in ('embed', 'total') else k]:.3e}" for k, e in errs.items()))
    oks = [note(f"oracle end to end {k} {g}", e, bars["resid" if k in ("embed", "total") else k]) for k, e in errs.items()]
    assert all(oks), (errs, bars)
    # 5: conservation on the engine: resid[:, L] + the b_U difference is the logit difference of Model.forward
    if pos_key is None:
        bU = tiny_model.weights.b_unembed.double().cpu().numpy()
        for s, ids in enumerate(seqs):
            lg = tiny_model.forward(ids, last_only=True)[0, 0].double().cpu().numpy()
            want = lg[TARGETS[s]] - (lg[CONTRAST[s]] if ct else 0.0)
            got = resid[s, -1] + bU[TARGETS[s]] - (bU[CONTRAST[s]] if ct else 0.0)
            assert note(f"conservation vs Model.forward {g}", abs(got - want), bars["resid"]), (s, got, want, bars["resid"])


def lens_checks(model, name, q64_p64_bars, pos, exact_rows):
    (q64, p64, bars) = q64_p64_bars
    cfg = model.cfg
    seqs = ragged_prompts(cfg, LENS)
    n, nl = len(seqs), cfg.n_layers
    trace = filled_trace(model, seqs)
    prob, top = trace.logit_lens(list(TARGETS), pos=pos, topk=TOPK)
    assert tuple(prob.shape) == (n, nl + 1) and tuple(top.shape) == (n, nl + 1, TOPK) and top.dtype == torch.int32
    prob_h, top_h = prob.cpu().numpy(), top.cpu().numpy()
    qpos = [len(s) - 1 for s in seqs] if pos is None else list(pos)
    if pos is None:  # row L is the model's own last-position distribution
        clean = model.forward_clean(seqs, targets=list(TARGETS), topk=TOPK)
        pc = clean["prob"].cpu().numpy()
        assert note(f"lens row L vs forward_clean / 1e-4 max {name}", np.abs(prob_h[:, nl] - pc).max(), FP32_TOL * pc.max())
    # the lens is decode_rows of the exported rows
    rows = torch.as_tensor([o + q for o, q in zip(trace.seq_offsets, qpos)], device=model.device)
    x = torch.stack([trace.resid_pre(l)[rows] for l in range(nl + 1)], 1)  # [n][L + 1][d]
    p_all, t_all = model.decode_rows(x.reshape(-1, cfg.d_model), targets=np.repeat(TARGETS, nl + 1), topk=TOPK)
    if exact_rows:  # same rows, same order, same launch shape: bit for bit
        assert (bits(p_all.cpu().numpy()) == bits(prob_h.reshape(-1))).all()
        assert (t_all.cpu().numpy() == top_h.reshape(-1, TOPK)).all()
    else:
        assert note(f"lens vs decode_rows / 1e-4 max {name}", np.abs(p_all.cpu().numpy() - prob_h.reshape(-1)).max(),
                    FP32_TOL * prob_h.max())
    for l in range(nl + 1):  # layer by layer: another launch shape
        pl, _ = model.decode_rows(x[:, l].contiguous(), targets=list(TARGETS))
        assert note(f"lens vs decode_rows / 1e-4 max {name}", np.abs(pl.cpu().numpy() - prob_h[:, l]).max(),
                    FP32_TOL * prob_h.max())
    only_top = trace.logit_lens(pos=pos, topk=TOPK)
    assert only_top[0] is None and (only_top[1].cpu().numpy() == top_h).all()
    if q64 is None:
        return
    # against the fp64 oracle
    want = p64[np.arange(n)[:, None], np.arange(nl + 1)[None], np.asarray(TARGETS)[:, None]]
    err = np.abs(prob_h - want).max()
    print(f"logit lens vs fp64 oracle ({name}, pos {pos}): err {err:.3e}, bar {bars['prob']:.3e}")
    assert note(f"lens prob vs oracle {name}", err, bars["prob"])
    keep, ids = robust_topk_rows(q64[4], TOPK, bars["logit"])
    assert (~keep).mean() <= 0.10, "choose other prompts: the fp64 oracle has near-ties at the top-k edge"
    for s in range(n):
        for l in range(nl + 1):
            if keep[s, l]:
                assert set(top_h[s, l].tolist()) == set(ids[s, l].tolist()), (s, l, top_h[s, l], ids[s, l])
    # the documented order (descending): where the fp64 oracle separates every rank up to k + 1
    ordered = ordered_topk_rows(q64[4], TOPK, bars["logit"])
    assert ordered.mean() >= 0.5, "choose other prompts: too few rows with a determined order"
    assert (top_h[ordered] == ids[ordered]).all(), (top_h[ordered], ids[ordered])


@pytest.mark.parametrize("pos_key", (None, "mid"))
def test_lens_and_decode(tiny_model, tiny_cfg, tiny_sd, tokenizer, pos_key):
    data = oracle_data(tiny_cfg, tiny_sd, tokenizer, pos_key, None)
    lens_checks(tiny_model, tiny_model.gemm, data, None if pos_key is None else list(MID), exact_rows=True)


def test_lens_and_decode_on_an_uncentred_trace(exact16_model):
    """The exact-fp16 model has other weights than the oracle's: the internal checks alone; its export is
    re-centred, so decode_rows sees other input bits than the lens."""
    lens_checks(exact16_model, "exact-fp16", (None, None, None), None, exact_rows=False)


def test_decode_rows_beyond_one_final_chunk(tiny_cfg, tiny_sd, tokenizer):
    """More rows than one chunk of the final stage (1,024 rows on the f32 path, which keeps a [rows][V] logit
    scratch): every chunk decodes its own rows.  Against the same rows decoded in two launches that each fit
    one chunk, against single rows, and against softmax(ln_final(x) W_U + b_U) in fp64 from the model's own
    fp32 weights."""
    m = tvr_amd.Model.from_hf_state_dict(tiny_cfg, tiny_sd, device="cuda", tokenizer=tokenizer, gemm="f32")
    n, d, V = 1024 + 37, tiny_cfg.d_model, tiny_cfg.d_vocab
    g = torch.Generator().manual_seed(5)
    rows = (torch.randn(n, d, generator=g) * torch.exp2(torch.randint(-3, 4, (n, 1), generator=g).float())).cuda()
    tg = torch.randint(0, V, (n,), generator=g).tolist()
    prob, top = m.decode_rows(rows, targets=tg, topk=TOPK)
    assert tuple(prob.shape) == (n,) and tuple(top.shape) == (n, TOPK)
    x = rows.double().cpu()
    xc = x - x.mean(-1, keepdim=True)
    xn = xc / (xc.pow(2).mean(-1, keepdim=True) + tiny_cfg.ln_eps).sqrt()
    logits = xn @ m.weights.w_unembed_t.double().cpu().T + m.weights.b_unembed.double().cpu()
    p64 = torch.softmax(logits, -1)
    want = p64[torch.arange(n), torch.as_tensor(tg)].numpy()
    prob_h, top_h = prob.cpu().numpy(), top.cpu().numpy()
    tol = FP32_TOL * want.max()
    assert note("decode_rows 1061 rows vs fp64 / 1e-4 max f32", np.abs(prob_h - want).max(), tol)
    assert note("decode_rows 1061 rows vs fp64 / 1e-4 max f32", np.abs(prob_h[1024:] - want[1024:]).max(), tol)  # the second chunk
    lg = logits.numpy()
    ordered = ordered_topk_rows(lg, TOPK, 1e-3 * np.abs(lg).max())
    assert ordered[1024:].any() and ordered.mean() > 0.5
    ids = np.argsort(-lg, -1)[:, :TOPK]
    assert (top_h[ordered] == ids[ordered]).all()
    # the same rows in launches of one chunk each, and row by row across the chunk edge
    for a, b in ((0, 1024), (1024, n), (600, 1061)):
        pa, ta = m.decode_rows(rows[a:b].contiguous(), targets=tg[a:b], topk=TOPK)
        assert np.abs(pa.cpu().numpy() - prob_h[a:b]).max() <= tol
        assert (ta.cpu().numpy()[ordered[a:b]] == top_h[a:b][ordered[a:b]]).all()
    for i in (0, 1023, 1024, 1025, n - 1):
        pi, ti = m.decode_rows(rows[i:i + 1].contiguous(), targets=tg[i:i + 1], topk=TOPK)
        assert abs(float(pi[0]) - prob_h[i]) <= tol
        assert not ordered[i] or (ti.cpu().numpy()[0] == top_h[i]).all()


def test_operators_check_widths_against_the_model(tiny_model):
    """A direct torch.ops.tvr call with a wrong width is refused before the engine is reached."""
    cfg, ops, h = tiny_model.cfg, tiny_model._ops, tiny_model._h.value
    d, H = cfg.d_model, cfg.n_heads
    z = torch.zeros(3, d, device="cuda")
    with pytest.raises(ValueError, match=r"\[n, d_model\]"):
        ops.head_attribution(h, 0, z[:, :d - 16].contiguous(), z[:, :d - 16].contiguous(), d, H, torch.zeros(3, H, device="cuda"))
    with pytest.raises(ValueError, match=r"\[n, n_heads\]"):
        ops.head_attribution(h, 0, z, z, d, H, torch.zeros(3, H + 1, device="cuda"))
    with pytest.raises(ValueError, match=r"rows must be \[n, d_model\]"):
        ops.decode_rows(h, torch.zeros(3, d + 4, device="cuda"), None, 1, d, None,
                        torch.zeros(3, 1, dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------ 7: the façade
FACADE_SEED, N_PROMPTS, LEN_PROMPT, TOP_N = 11, 6, 9, 2


def facade_inputs(cfg):
    """Token-id prompts and answers in the forms normalize_cie_inputs accepts (id lists; answers as ints and as
    token lists).  No string is encoded: the session's synthetic tokenizer gives a piece it has not seen a
    hashed id and remembers it, which would change what later tests of the session decode."""
    prompts = ragged_prompts(cfg, (LEN_PROMPT,) * N_PROMPTS, seed=FACADE_SEED)
    g = torch.Generator().manual_seed(FACADE_SEED + 1)
    ids = torch.randint(1, cfg.d_vocab, (N_PROMPTS,), generator=g).tolist()
    return prompts, [t if i % 2 else [t, 0] for i, t in enumerate(ids)]


def test_facade_against_the_oracle(tiny_model, tiny_cfg, tiny_sd, tokenizer):
    cfg, g = tiny_cfg, tiny_model.gemm
    prompts, answers = facade_inputs(cfg)
    seqs, tg = experiments.normalize_cie_inputs(tiny_model, prompts, answers)
    if "facade" not in _oracle_cache:
        if "pair" not in _oracle_cache:
            _oracle_cache["pair"] = oracle_pair(cfg, tiny_sd, tokenizer)
        o32, o64 = _oracle_cache["pair"]
        qpos = [len(s) - 1 for s in seqs]
        _oracle_cache["facade"] = (oracle_quantities(o32, seqs, qpos, tg, None), oracle_quantities(o64, seqs, qpos, tg, None))
    q32, q64 = _oracle_cache["facade"]
    floor = C.floor_of(q64[5])
    bar_h = max(4.0 * np.abs(q32[0] - q64[0]).max(), floor)
    bar_r = max(4.0 * np.abs(q32[2] - q64[2]).max(), floor)
    bar_rest = max(4.0 * np.abs(q32[1] - q64[1]).max(), floor)
    out = experiments.head_logit_attribution(prompts, answers, model=tiny_model)
    assert isinstance(out, experiments.HeadLogitAttribution)
    assert tuple(out.heads.shape) == (cfg.n_layers, cfg.n_heads) and tuple(out.rest.shape) == (cfg.n_layers,)
    heads, rest = out.heads.double().cpu().numpy(), out.rest.double().cpu().numpy()
    embed, total = float(out.embed), float(out.total)
    # means over prompts: the error of a mean is at most the largest error of its terms
    assert note(f"facade heads {g}", np.abs(heads - q64[0].mean(0)).max(), bar_h)
    assert note(f"facade rest {g}", np.abs(rest - q64[1].mean(0)).max(), bar_rest)
    assert note(f"facade embed {g}", abs(embed - q64[2][:, 0].mean()), bar_r)
    assert note(f"facade total {g}", abs(total - q64[2][:, -1].mean()), bar_r)
    # the parts add up: rest is resid[l + 1] - resid[l] - the heads, so the sum telescopes up to fp32 rounding of
    # the 2 L + L H + 1 additions involved, each at most 2^-24 of the magnitudes summed
    mags = np.abs(heads).sum() + 2 * np.abs(q64[2].mean(0)).sum() + np.abs(rest).sum()
    assert abs(heads.sum() + rest.sum() + embed - total) <= 4 * (2 * cfg.n_layers + cfg.n_layers * cfg.n_heads + 1) * C.EPS24 * mags
    # the selection: the oracle's top heads, where the oracle separates rank n from rank n + 1
    ref = q64[0].mean(0)
    order = np.sort(ref.ravel())[::-1]
    assert order[TOP_N - 1] - order[TOP_N] > 2 * bar_h, "choose another FACADE_SEED: the oracle has no gap"
    want = {(int(i) // cfg.n_heads, int(i) % cfg.n_heads) for i in np.argsort(-ref.ravel())[:TOP_N]}
    assert set(experiments.top_attribution_heads(out.heads, TOP_N)) == want
    # with contrast answers: the same call on the differences (engine-internal: against Trace.logit_attribution)
    contrast = [[t] for t in CONTRAST[:1] * len(tg)]
    out_c = experiments.head_logit_attribution(prompts, answers, model=tiny_model, contrast_answers=contrast)
    trace = filled_trace(tiny_model, seqs)
    h, r = trace.logit_attribution(tg, contrast=[CONTRAST[0]] * len(tg))
    assert (bits((h.sum(0) / len(tg)).cpu().numpy()) == bits(out_c.heads.cpu().numpy())).all()
    assert float(out_c.total) == float(r.sum(0)[-1] / len(tg))

    # logit_lens_by_layer: the share of prompts with the answer in the top k, and the mean probability
    acc, prob = experiments.logit_lens_by_layer(prompts, answers, model=tiny_model, topk=TOPK)
    assert tuple(acc.shape) == (cfg.n_layers + 1,) and tuple(prob.shape) == (cfg.n_layers + 1,)
    p32 = torch.softmax(torch.from_numpy(q32[4]), -1).numpy()
    p64 = torch.softmax(torch.from_numpy(q64[4]), -1).numpy()
    bar_p = max(4.0 * np.abs(p32 - p64).max(), 2.0 ** -22)
    pt = p64[np.arange(len(tg)), :, np.asarray(tg)]  # [n][L + 1]
    assert note(f"facade lens prob {g}", np.abs(prob.double().cpu().numpy() - pt.mean(0)).max(), bar_p)
    bar_logit = max(4.0 * np.abs(q32[4] - q64[4]).max(), 2.0 ** -22 * np.abs(q64[4]).max())
    keep, ids = robust_topk_rows(q64[4], TOPK, bar_logit)
    hit = (ids == np.asarray(tg)[:, None, None]).any(-1)  # [n][L + 1]
    lo = (hit & keep).sum(0) / len(tg)
    hi = (hit | ~keep).sum(0) / len(tg)
    a = acc.double().cpu().numpy()
    assert (a >= lo - 1e-9).all() and (a <= hi + 1e-9).all(), (a, lo, hi)
    assert (~keep).mean() <= 0.10

    # decode_vectors: the top-k token strings of each row, here the final residual rows of the prompts
    rows = torch.as_tensor([o + n - 1 for o, n in zip(trace.seq_offsets, map(len, seqs))], device="cuda")
    table = experiments.decode_vectors(trace.resid_pre(cfg.n_layers)[rows], TOPK, model=tiny_model)
    assert len(table) == len(seqs) and all(len(r) == TOPK for r in table)
    for s in range(len(seqs)):
        if keep[s, -1]:
            assert set(table[s]) == {tiny_model.to_string(int(i)) for i in ids[s, -1]}
    one = experiments.decode_vectors(trace.resid_pre(cfg.n_layers)[rows[0]], 1, model=tiny_model)  # a single vector
    assert len(one) == 1 and len(one[0]) == 1
    if robust_topk_rows(q64[4], 1, bar_logit)[0][0, -1]:
        assert one == [table[0][:1]]
