"""``attention_pattern_kernel`` alone (``tvr_attention_pattern``), on a trace
(``tvr_trace_capture_pattern``, ``Trace.q / k / v``) and through the façade
(``head_attention_profile``), against the fp64 references of
tests/pattern_cases.py and the oracle.

Primitive: one small model per (d_head, n_heads) of attention_cases.MODELS (its
weights are never used), TL's fp32 rotary tables passed in.  Every launch
(``run``) checks what must NOT be written, bit for bit — guard rows before and
after out_pattern / out_mass — that columns (qpos, ld) are +0.0 and that no NaN
comes out although every Q row but the query's and every row between the
sequences is NaN.  Bars (pattern_cases.bar): 4 x the larger error of two fp32
restatements of the case, floored at 2^-22; ``select`` is bit-exact; ``uniform``
is fl(1 / fl(q + 1)) bit for bit (the kernel normalises by IEEE division, not
by reciprocal-and-multiply); tied keys of ``huge`` get equal bits; rows sum to 1
within (q + 1) 2^-24; the mass is within (q + 1) 2^-24 of the fp64 class sums
of the GPU's own pattern (any-order fp32 summation of non-negative terms that
sum to at most 1).

Trace path: the pattern against the fp64 reference built from the trace's OWN
fp32 hook_q / hook_k at the kernel bar plus the table allowance 2 x shift of
test_gpu_attention.py::test_model_tables (the engine's powf / division / cosf
may each differ from torch's by an ulp), on every GEMM path; end to end against
the fp64 oracle at max(4 x |pattern(fp32 oracle) - pattern(fp64 oracle)|, 2^-22).

Measured on an MI355X by this file (printed at its end), worst max |p - p64| /
bar over every kind and both ld of a (d_head, T), T = 1 / 15 / 16 / 17 / 63 / 64
/ 65 / 129 / 300:
  d_head  16: 0.000 0.241 0.376 0.250 0.271 0.291 0.292 0.241 0.166
  d_head  64: 0.000 0.204 0.250 0.205 0.132 0.195 0.179 0.158 0.106
  d_head  80: 0.000 0.121 0.267 0.246 0.256 0.204 0.269 0.238 0.222
  d_head 128: 0.000 0.303 0.250 0.349 0.514 0.254 0.336 0.320 0.155
and 0.024 at d_head 64, T = 2048 (the bar is its 2^-22 floor there).  select
bitwise at every d_head.  Trace against its own Q / K: f32 0.095, x2f16
0.075, x3bf16 0.109, exact-fp16 0.110.  End to end against the fp64 oracle
(bar 1.67e-6 .. 1.78e-6, the margin of 4 holds): f32 0.264, x2f16 0.192, x3bf16
0.204; head_attention_profile f32 0.080, x2f16 0.066, x3bf16 0.098; hook_q / k /
v relative error at most 5e-7 (bar 1e-4).  The whole file (43 tests) runs in
about 3 s.

A miss these tests found while the kernel was written: with each key's dot
product as ONE serial chain of d_head fmas the worst ratio was 1.132 at d_head
128 (random_gain, T = 17: 7.89e-7 against a bar of 6.97e-7) and 0.995 at d_head
80.  The dot product now runs as four chains (dim e in chain e % 4) summed
pairwise, which is what the figures above measure.
"""
import collections
import functools
import gc
import math
import random
import time

import numpy as np
import pytest
import torch

import attention_cases as A
import pattern_cases as P
import tvr_amd
from tvr_amd import _lib as L, experiments, prompts
from tvr_amd.prompts import ROLES

pytestmark = [pytest.mark.gpu]

G = 2                  # guard rows before and after every output
NAN_BITS = 0x7FC00000  # torch.full(nan)
EPS24 = 2.0 ** -24
FP32_TOL = 1e-4  # tests/test_gpu_task_vectors.py: an exported activation
MODEL_IDS = [f"dh{dh}h{h}" for dh, h in A.MODELS]
ARROW = tvr_amd.tasks.ARROW

_worst = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _module():
    t0 = time.time()
    yield
    for form, r in sorted(_worst.items()):
        print(f"\nattention pattern, worst err / bar: {form:34s} {r:.3f}", end="")
    print(f"\nattention pattern tests: {time.time() - t0:.1f} s from the first test to the last")
    for cache in (_ref, _ctx):
        cache.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


class Ctx:
    def __init__(self, DH, H, n_ctx=A.N_CTX):
        self.DH, self.H, self.d = DH, H, DH * H
        cfg = tvr_amd.config.PythiaConfig(1, self.d, H, A.D_MLP, 64, n_ctx=n_ctx, name=f"pattern-{DH}x{H}")
        w = tvr_amd.weights.synth_engine_weights(cfg, seed=1, device="cuda")
        self.model = tvr_amd.Model(cfg, w, tokenizer=tvr_amd.tokenizer.SyntheticTokenizer(512), device="cuda", gemm="f32")
        self.lib, self.h = self.model._lib, self.model._h
        self.cos, self.sin = A.tables(DH, n_ctx)
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
    """(case, p64, bar): computed once, shared by every test."""
    case = P.make(kind, model[0], model[1], T)
    c = _ctx(model)
    p64 = P.reference(case, c.cos, c.sin)
    return case, p64, P.bar(case, c.cos, c.sin, p64)[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def guarded(shape):
    return torch.full((shape[0] + 2 * G,) + tuple(shape[1:]), float("nan"), dtype=torch.float32, device="cuda")


def inner(t):
    """(pointer to the first row behind the guard, the guard rows' bits as a check)."""
    return t.data_ptr() + G * t.stride(0) * t.element_size()


def unguard(t, what):
    h = t.cpu().numpy()
    b = h.view(np.int32)
    assert (b[:G] == NAN_BITS).all() and (b[-G:] == NAN_BITS).all(), f"{what}: guard rows written"
    return h[G:-G].copy()


def call(ctx, case, cls, n_classes, pat, ld, mass, tables=True, qkv=None, rows=None, row0=None, qpos=None, n_seq=None):
    """tvr_attention_pattern with the case's arguments, any of them overridden; returns the status."""
    if not hasattr(case, "dev"):  # the inputs go to the device once per case
        case.dev = torch.from_numpy(case.qkv).cuda()
    row0 = case.row0 if row0 is None else np.asarray(row0, dtype=np.int32)
    qpos = case.qpos if qpos is None else np.asarray(qpos, dtype=np.int32)
    cls = None if cls is None else np.ascontiguousarray(cls, dtype=np.int32)
    return ctx.lib.tvr_attention_pattern(
        ctx.h, case.dev.data_ptr() if qkv is None else qkv, case.lay.rows if rows is None else rows,
        row0.ctypes.data, qpos.ctypes.data, case.lay.n_seq if n_seq is None else n_seq,
        None if cls is None else cls.ctypes.data, n_classes, pat, ld, mass,
        ctx.d_cos.data_ptr() if tables else None, ctx.d_sin.data_ptr() if tables else None, ctx.stream())


def run(ctx, case, ld=None, cls=None, n_classes=0, want_pattern=True, want_mass=False, tables=True):
    """One launch on guarded, NaN-filled outputs: (pattern [n_seq][H][ld] or None, mass [n_seq][H][C] or None).
    Asserts the guards, no NaN, and +0.0 in the columns beyond every query position."""
    n, H = case.lay.n_seq, case.n_heads
    ld = case.maxT if ld is None else ld
    pat = guarded((n, H, ld)) if want_pattern else None
    mass = guarded((n, H, n_classes)) if want_mass else None
    rc = call(ctx, case, cls, n_classes, None if pat is None else inner(pat), ld, None if mass is None else inner(mass),
              tables)
    L.check(rc, "tvr_attention_pattern")
    p = m = None
    if pat is not None:
        p = unguard(pat, "out_pattern")
        assert not np.isnan(p).any(), "NaN in the pattern: a row or a Q that is not the sequence's was read"
        for s, q in enumerate(case.qpos):
            assert (bits(p[s, :, q + 1:]) == 0).all(), "columns (qpos, ld) must be +0.0"
    if mass is not None:
        m = unguard(mass, "out_mass")
        assert not np.isnan(m).any(), "NaN in the mass"
    return p, m


def check_rows_sum_to_one(p, qpos):
    for s, q in enumerate(qpos):
        dev = np.abs(p[s].astype(np.float64).sum(-1) - 1.0).max()
        assert dev <= (q + 1) * EPS24, (s, q, dev)


# ------------------------------------------------------------------------------ 1: accuracy and exact answers
def test_accuracy_against_fp64(ctx):
    model = (ctx.DH, ctx.H)
    for T in P.ALL_T:
        for kind in P.KINDS:
            case, p64, bar = _ref(model, kind, T)
            for ld in (T, T + 3):
                p, _ = run(ctx, case, ld=ld)
                err = P.max_err(p[..., :T], p64)
                key = f"primitive dh {ctx.DH:3d} T {T:3d}"
                _worst[key] = max(_worst[key], err / bar)
                assert err <= bar, (kind, T, ld, err, bar)
                check_rows_sum_to_one(p, case.qpos)
            if kind == "uniform":  # Q = 0: every seen key is fl(1 / fl(q + 1)), bit for bit (IEEE division)
                for s, q in enumerate(case.qpos):
                    want = np.float32(1.0) / np.float32(q + 1)
                    assert (bits(p[s, :, :q + 1]) == bits(want)).all(), (T, s)
            if kind == "huge":  # the keys of a block of 8 inside one chunk of 128 are exactly tied
                for s, q in enumerate(case.qpos):
                    nb = (q + 1) // 8
                    if nb:
                        blk = bits(p[s, :, :8 * nb]).reshape(ctx.H, nb, 8)
                        assert (blk == blk[:, :, :1]).all(), (T, s)


def test_select_is_bitwise(ctx):
    """1.0 at min(pi, qpos) and +0.0 elsewhere, for every head and rotation of the families over the heads."""
    for T in P.ALL_T:
        for rot in A.SELECT_ROTS:
            case = P.make("select", ctx.DH, ctx.H, T, rot=rot)
            for ld in (T, T + 3):
                p, _ = run(ctx, case, ld=ld)
                assert (bits(p) == bits(P.one_hot(case, ld))).all(), (T, rot, ld)
    _worst[f"primitive dh {ctx.DH:3d} select: bitwise"] = 0.0


def test_model_tables(ctx):
    """cos_t = sin_t = NULL (the tables tvr_model_create computes) against TL's: the allowance of
    test_gpu_attention.py::test_model_tables, on the pattern."""
    case, p64, bar = _ref((ctx.DH, ctx.H), "rotary_only", 300)
    shift = table_shift(case, ctx.DH)
    own, _ = run(ctx, case, tables=False)
    assert 0 < shift and P.max_err(own, p64) <= 2 * shift + bar


def test_full_context():
    """2048 keys, the Pythias' n_ctx: 32 passes of the lanes over the keys and 8 KiB of scores per wave."""
    DH, H, T = 64, 4, 2048
    ctx = Ctx(DH, H, n_ctx=T)
    for kind in ("random", "huge"):
        case = P.make(kind, DH, H, T)
        p64 = P.reference(case, ctx.cos, ctx.sin)
        bar = P.bar(case, ctx.cos, ctx.sin, p64)[0]
        p, _ = run(ctx, case, ld=T + 1)
        err = P.max_err(p[..., :T], p64)
        _worst["primitive dh  64 T 2048"] = max(_worst["primitive dh  64 T 2048"], err / bar)
        assert err <= bar, (kind, err, bar)
        check_rows_sum_to_one(p, case.qpos)
    blk = bits(p[0, :, :T]).reshape(H, T // 8, 8)  # huge: the keys of a block of 8 are exactly tied
    assert (blk == blk[:, :, :1]).all()


def table_shift(case, DH, n_ctx=A.N_CTX):
    """What moving TL's fp32 frequencies by 2 ulp does to the fp64 reference of the case."""
    f = A.tl_freq32(DH)
    pa = P.reference(case, *A.tables_from_freq(f, n_ctx))
    pb = P.reference(case, *A.tables_from_freq(f * (1 + 2.0 ** -22), n_ctx))
    return P.max_err(pb, pa)


# ------------------------------------------------------------------------------ 2: the mass
def test_mass(ctx):
    model = (ctx.DH, ctx.H)
    C = P.N_CLASSES
    for T in P.ALL_T:
        case, _, _ = _ref(model, "random_gain", T)
        cls = P.classes(case)
        alone, _ = run(ctx, case)
        p, m = run(ctx, case, cls=cls, n_classes=C, want_mass=True)
        assert (bits(p) == bits(alone)).all(), "asking for the mass changed the pattern"
        want = P.class_sums(p, case, cls)
        for s, q in enumerate(case.qpos):
            assert np.abs(m[s].astype(np.float64) - want[s]).max() <= (q + 1) * EPS24, (T, s)
        empty = want == 0  # no key of the class among the seen ones (p > 0 for every seen key of these cases)
        assert empty[1, :, 2].all() and empty[2, :, 0].all() and empty[2, :, 2].all()
        assert (bits(m)[empty] == 0).all(), "an empty class must be +0.0"
        p2, m2 = run(ctx, case, cls=cls, n_classes=C, want_mass=True)
        assert (bits(p2) == bits(p)).all() and (bits(m2) == bits(m)).all(), "two runs differ"
        _, m3 = run(ctx, case, cls=cls, n_classes=C, want_pattern=False, want_mass=True)
        assert (bits(m3) == bits(m)).all(), "the mass depends on whether the pattern is written"
        # the classes given but no mass asked for: the pattern alone
        p4, _ = run(ctx, case, cls=cls, n_classes=C)
        assert (bits(p4) == bits(p)).all()


# ------------------------------------------------------------------------------ 3: the trace path
LENS = (1, 5, 17, 33)
MID = (0, 2, 8, 20)


def ragged_prompts(cfg, lens, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [[0] + torch.randint(1, cfg.d_vocab, (n - 1,), generator=g).tolist() for n in lens]


def filled_trace(model, seqs, defer=False):
    trace = model.trace(len(seqs), sum(map(len, seqs)))
    model.forward_clean(seqs, trace=trace, defer=defer)
    return trace


@pytest.fixture(scope="module")
def exact16_model(tiny_cfg, tokenizer):
    """fp16-valued weights: the exact-fp16 GEMMs are bound (as tests/test_gpu_task_vectors.py builds it)."""
    sd = tvr_amd.weights.synth_hf_state_dict(tiny_cfg, seed=0, std=0.3, fp16=True)
    m = tvr_amd.Model.from_hf_state_dict(tiny_cfg, sd, device="cuda", tokenizer=tokenizer, gemm="x2f16")
    assert m.exact16
    return m


def check_trace_against_its_own_qk(model, what):
    cfg = model.cfg
    Lr, H, DH = cfg.n_layers, cfg.n_heads, cfg.d_head
    seqs = ragged_prompts(cfg, LENS)
    cos, sin = A.tables(DH, n_ctx=cfg.n_ctx, base=cfg.rotary_base)
    trace = filled_trace(model, seqs)
    results = {}
    for pos in (None, MID):
        qpos = [len(s) - 1 for s in seqs] if pos is None else list(pos)
        pat = trace.attention_pattern(pos).cpu().numpy()
        assert pat.shape == (len(seqs), Lr, H, max(qpos) + 1) and not np.isnan(pat).any()
        for l in range(Lr):
            case = P.from_rows(trace.q(l).cpu().numpy(), trace.k(l).cpu().numpy(), LENS, qpos, DH, H)
            p64 = P.reference(case, cos, sin)
            bar = P.bar(case, cos, sin, p64)[0] + 2 * table_shift(case, DH, cfg.n_ctx)
            err = P.max_err(pat[:, l], p64[..., :pat.shape[-1]])
            key = f"trace {what}"
            _worst[key] = max(_worst[key], err / bar)
            assert err <= bar, (what, pos, l, err, bar)
            check_rows_sum_to_one(pat[:, l], qpos)
            for s, q in enumerate(qpos):
                assert (bits(pat[s, l, :, q + 1:]) == 0).all()
        results[pos] = pat
    # a deferred clean forward: the call must run it first, and gives the same bits
    for pos in (None, MID):
        deferred = filled_trace(model, seqs, defer=True)
        assert (bits(deferred.attention_pattern(pos).cpu().numpy()) == bits(results[pos])).all()
    # the mass on the trace: its own pattern's class sums, classes as one list per sequence
    classes = [[(j * 5 + s) % 4 - 1 for j in range(len(q))] for s, q in enumerate(seqs)]
    mass = trace.attention_mass(classes, 3).cpu().numpy()
    pat = results[None]
    for s, q in enumerate(seqs):
        c = np.asarray(classes[s])
        for k in range(3):
            want = pat[s, :, :, :len(q)].astype(np.float64)[..., c == k].sum(-1)
            assert np.abs(mass[s, :, :, k] - want).max() <= len(q) * EPS24
    flat = trace.attention_mass([c for cs in classes for c in cs], 3).cpu().numpy()
    assert (bits(flat) == bits(mass)).all()


def test_trace_pattern_against_its_own_qk(tiny_model):
    check_trace_against_its_own_qk(tiny_model, tiny_model.gemm)


def test_trace_pattern_against_its_own_qk_exact16(exact16_model):
    check_trace_against_its_own_qk(exact16_model, "exact16")


def oracle_qkv_pattern(oracle, ids, pos=None):
    """Per layer (q, k, v [T, d] before rotary, pattern [H, pos + 1]) recomputed from the oracle's cached
    hook_resid_pre with its own _ln_pre, W_Q / W_K / W_V, biases and _rotate."""
    _, cache = oracle.run_with_cache(torch.tensor([ids]))
    pos = len(ids) - 1 if pos is None else pos
    out = []
    for l in range(oracle.cfg.n_layers):
        b = oracle.w["blocks"][l]
        x = oracle._ln_pre(cache[f"blocks.{l}.hook_resid_pre"])
        q = torch.einsum("bpd,hde->bphe", x, b["W_Q"]) + b["b_Q"]
        k = torch.einsum("bpd,hde->bphe", x, b["W_K"]) + b["b_K"]
        v = torch.einsum("bpd,hde->bphe", x, b["W_V"]) + b["b_V"]
        sc = torch.einsum("bqhe,bkhe->bhqk", oracle._rotate(q), oracle._rotate(k)) / math.sqrt(oracle.cfg.d_head)
        p = torch.softmax(sc[0, :, pos, :pos + 1], dim=-1)
        out.append(tuple(t[0].reshape(len(ids), -1) for t in (q, k, v)) + (p,))
    return out


def rel_err(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def test_trace_qkv_against_the_oracle(tiny_model, tiny_oracle64):
    seqs = ragged_prompts(tiny_model.cfg, LENS)
    trace = filled_trace(tiny_model, seqs)
    off = np.concatenate([[0], np.cumsum(LENS)])
    want = [oracle_qkv_pattern(tiny_oracle64, s) for s in seqs]
    for l in range(tiny_model.cfg.n_layers):
        for i, (name, got) in enumerate((("q", trace.q(l)), ("k", trace.k(l)), ("v", trace.v(l)))):
            assert tuple(got.shape) == (sum(LENS), tiny_model.cfg.d_model)
            ref = torch.cat([w[l][i] for w in want])
            e = rel_err(got, ref)
            key = f"hook_q / k / v rel err / 1e-4 {tiny_model.gemm}"
            _worst[key] = max(_worst[key], e / FP32_TOL)
            assert e <= FP32_TOL, (name, l, e)
    assert off[-1] == trace.q(0).shape[0]
    with pytest.raises(ValueError, match="bad hook/layer"):
        trace.q(tiny_model.cfg.n_layers)  # hook_q has no layer n_layers (hook_resid_pre does)


def oracle_bar(oracle32, oracle64, seqs, qpos):
    """(bar, fp64 patterns per prompt [L][H][q + 1]) from the two oracles alone."""
    worst, p64s = 0.0, []
    for ids, q in zip(seqs, qpos):
        p32 = [t[3] for t in oracle_qkv_pattern(oracle32, ids, q)]
        p64 = [t[3] for t in oracle_qkv_pattern(oracle64, ids, q)]
        worst = max(worst, max((a.double() - b).abs().max().item() for a, b in zip(p32, p64)))
        p64s.append(torch.stack(p64).numpy())
    return max(4.0 * worst, 2.0 ** -22), p64s


def test_pattern_against_the_oracle(tiny_model, tiny_oracle, tiny_oracle64):
    seqs = ragged_prompts(tiny_model.cfg, LENS)
    for pos in (None, MID):
        qpos = [len(s) - 1 for s in seqs] if pos is None else list(pos)
        bar, p64s = oracle_bar(tiny_oracle, tiny_oracle64, seqs, qpos)
        pat = filled_trace(tiny_model, seqs).attention_pattern(pos).cpu().numpy()
        err = max(np.abs(pat[s, :, :, :q + 1] - p64s[s]).max() for s, q in enumerate(qpos))
        key = f"oracle end to end {tiny_model.gemm}"
        _worst[key] = max(_worst[key], err / bar)
        print(f"pattern vs fp64 oracle ({tiny_model.gemm}, pos {pos}): err {err:.3e}, bar {bar:.3e}, ratio {err / bar:.3f}")
        assert err <= bar, (tiny_model.gemm, pos, err, bar)


def test_bf16_path_runs(tiny_cfg, tiny_sd, tokenizer):
    """Not fp32-accurate, so not held to the bar: the rows sum to 1 and the zero fill holds."""
    m = tvr_amd.Model.from_hf_state_dict(tiny_cfg, tiny_sd, device="cuda", tokenizer=tokenizer, gemm="bf16")
    seqs = ragged_prompts(tiny_cfg, LENS)
    trace = filled_trace(m, seqs)
    for pos in (None, MID):
        qpos = [len(s) - 1 for s in seqs] if pos is None else list(pos)
        pat = trace.attention_pattern(pos).cpu().numpy()
        assert not np.isnan(pat).any()
        for l in range(tiny_cfg.n_layers):
            check_rows_sum_to_one(pat[:, l], qpos)
        for s, q in enumerate(qpos):
            assert (bits(pat[s, :, :, q + 1:]) == 0).all()


# ------------------------------------------------------------------------------ 4: the façade
PROFILE_SEED, N_CONTEXTS, LEN_CONTEXTS, TOP_N = 3, 8, 2, 2


def test_head_attention_profile_against_the_oracle(tiny_model, tiny_oracle, tiny_oracle64):
    contexts = list(tvr_amd.tasks.letter_to_caps)
    random.seed(PROFILE_SEED)
    seqs, roles = prompts.sample_icl_prompts_with_roles(tiny_model, contexts, ARROW, ",", N_CONTEXTS, LEN_CONTEXTS)
    random.seed(PROFILE_SEED)
    prof = experiments.head_attention_profile(contexts, ARROW, ",", model=tiny_model, num_contexts=N_CONTEXTS,
                                              len_contexts=LEN_CONTEXTS)
    cfg = tiny_model.cfg
    assert tuple(prof.shape) == (cfg.n_layers, cfg.n_heads, len(ROLES))
    # the reference's way: one run_with_cache per prompt, the pattern at the last position summed by role
    bar, p64s = oracle_bar(tiny_oracle, tiny_oracle64, seqs, [len(s) - 1 for s in seqs])
    ref = np.zeros((cfg.n_layers, cfg.n_heads, len(ROLES)))
    for p64, r in zip(p64s, roles):
        r = np.asarray(r)
        for c in range(len(ROLES)):
            ref[:, :, c] += p64[:, :, r == c].sum(-1)
    ref /= N_CONTEXTS
    got = prof.double().cpu().numpy()
    err = np.abs(got - ref).max()
    key = f"head_attention_profile {tiny_model.gemm}"
    _worst[key] = max(_worst[key], err / bar)
    print(f"head_attention_profile ({tiny_model.gemm}): err {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    T = max(map(len, seqs))
    assert np.abs(got.sum(-1) - 1.0).max() <= T * EPS24
    # the selection: the reference's top heads, where the reference separates rank n from rank n + 1
    role = ROLES.index("demo_label")
    order = np.sort(ref[:, :, role].ravel())[::-1]
    assert order[TOP_N - 1] - order[TOP_N] > 2 * bar, "choose another PROFILE_SEED: the reference has no gap"
    want = {(int(i) // cfg.n_heads, int(i) % cfg.n_heads) for i in np.argsort(-ref[:, :, role].ravel())[:TOP_N]}
    assert set(experiments.top_attention_heads(prof, "demo_label", TOP_N)) == want


# ------------------------------------------------------------------------------ 5: validation
def test_invalid_arguments_launch_nothing():
    ctx = _ctx(A.MODELS[0])
    case, _, _ = _ref(A.MODELS[0], "random", 17)
    n, H, T, C = case.lay.n_seq, ctx.H, 17, P.N_CLASSES
    cls = P.classes(case)
    pat, mass = guarded((n, H, T)), guarded((n, H, C))
    po, mo = inner(pat), inner(mass)
    run(ctx, case)  # (the inputs are on the device from here on)
    qkv = case.dev.data_ptr()

    def refused(message, *a, **kw):
        rc = call(ctx, case, *a, **kw)
        err = ctx.lib.tvr_last_error().decode()
        assert rc == L.TVR_ERR_INVALID and err.startswith("tvr_attention_pattern: ") and message in err, (message, rc, err)

    bad_cls = cls.copy()
    bad_cls[case.row0[0] + 3] = C
    low_cls = cls.copy()
    low_cls[0] = -2
    refused("null qkv", cls, C, po, T, mo, qkv=0)
    refused("both null", cls, C, None, T, None)
    refused("out_mass needs cls", None, C, po, T, mo)
    refused("n_classes must be in [1, 64]", cls, 0, po, T, mo)
    refused("n_classes must be in [1, 64]", cls, 65, po, T, None)
    refused("outside [-1, n_classes)", bad_cls, C, po, T, mo)
    refused("outside [-1, n_classes)", low_cls, C, po, T, None)
    refused("n_seq must be positive", cls, C, po, T, mo, n_seq=0)
    refused("rows must be positive", cls, C, po, T, mo, rows=0)
    refused("qpos outside [0, n_ctx)", cls, C, po, T, mo, qpos=[-1, 8, 0])
    refused("qpos outside [0, n_ctx)", cls, C, po, A.N_CTX + 1, mo, qpos=[A.N_CTX, 8, 0])
    refused("ld must exceed", cls, C, po, T - 1, mo)
    refused("outside the qkv buffer", cls, C, po, T, mo, row0=[-1, 19, 37])
    refused("outside the qkv buffer", cls, C, po, T, mo, rows=int(case.row0[2]))
    refused("16-byte aligned", cls, C, po, T, mo, qkv=qkv + 4)
    rc = ctx.lib.tvr_attention_pattern(ctx.h, qkv, case.lay.rows, case.row0.ctypes.data, case.qpos.ctypes.data, n, None, 0,
                                       po, T, None, ctx.d_cos.data_ptr(), None, ctx.stream())
    assert rc == L.TVR_ERR_INVALID and "cos_t and sin_t" in ctx.lib.tvr_last_error().decode()
    rc = ctx.lib.tvr_attention_pattern(ctx.h, qkv, case.lay.rows, None, case.qpos.ctypes.data, n, None, 0, po, T, None,
                                       None, None, ctx.stream())
    assert rc == L.TVR_ERR_INVALID and "null row0 / qpos" in ctx.lib.tvr_last_error().decode()
    torch.cuda.synchronize()
    assert (pat.cpu().numpy().view(np.int32) == NAN_BITS).all() and (mass.cpu().numpy().view(np.int32) == NAN_BITS).all()
    # ld is not looked at when no pattern is asked for; and the model is still usable
    assert call(ctx, case, cls, C, None, 0, mo) == L.TVR_OK
    p, m = run(ctx, case, cls=cls, n_classes=C, want_mass=True)
    assert (bits(unguard(mass, "out_mass")) == bits(m)).all()


def test_invalid_trace_arguments_launch_nothing(tiny_model):
    cfg = tiny_model.cfg
    lib = tiny_model._lib
    seqs = ragged_prompts(cfg, LENS)
    n, tokens = len(seqs), sum(LENS)
    empty = tiny_model.trace(n, tokens)
    trace = filled_trace(tiny_model, seqs)
    ld, C = max(LENS), 3
    pat, mass = guarded((n, cfg.n_layers, cfg.n_heads, ld)), guarded((n, cfg.n_layers, cfg.n_heads, C))
    po, mo = inner(pat), inner(mass)
    cls = np.zeros(tokens, dtype=np.int32)
    st = tiny_model._stream()

    def refused(message, tr, pos, c, n_classes, p, ldv, m):
        pos = None if pos is None else np.asarray(pos, dtype=np.int32)
        rc = lib.tvr_trace_capture_pattern(tr._h, None if pos is None else pos.ctypes.data,
                                           None if c is None else c.ctypes.data, n_classes, p, ldv, m, st)
        err = lib.tvr_last_error().decode()
        assert rc == L.TVR_ERR_INVALID and err.startswith("tvr_trace_capture_pattern: ") and message in err, (message, rc, err)

    bad = cls.copy()
    bad[-1] = C
    refused("trace is empty", empty, None, cls, C, po, ld, mo)
    refused("both null", trace, None, cls, C, None, ld, None)
    refused("out_mass needs cls", trace, None, None, C, po, ld, mo)
    refused("n_classes must be in [1, 64]", trace, None, cls, 0, po, ld, mo)
    refused("n_classes must be in [1, 64]", trace, None, cls, 65, po, ld, mo)
    refused("outside [-1, n_classes)", trace, None, bad, C, po, ld, mo)
    refused("pos of sequence 1 out of range", trace, [0, 5, 0, 0], cls, C, po, ld, mo)
    refused("pos of sequence 0 out of range", trace, [-1, 0, 0, 0], cls, C, po, ld, mo)
    refused("ld must exceed", trace, None, cls, C, po, ld - 1, mo)
    torch.cuda.synchronize()
    assert (pat.cpu().numpy().view(np.int32) == NAN_BITS).all() and (mass.cpu().numpy().view(np.int32) == NAN_BITS).all()
    # the façade's own checks come first and raise ValueError as well
    with pytest.raises(ValueError, match="outside its sequence"):
        trace.attention_pattern([0, 5, 0, 0])
    with pytest.raises(ValueError, match="trace is empty"):
        empty.attention_pattern()
    # afterwards the trace and the model are still usable: a valid call on the same buffers
    rc = lib.tvr_trace_capture_pattern(trace._h, None, cls.ctypes.data, C, po, ld, mo, st)
    L.check(rc, "tvr_trace_capture_pattern")
    got = unguard(pat, "out_pattern")
    assert (bits(got) == bits(trace.attention_pattern().cpu().numpy())).all()
    m = unguard(mass, "out_mass")
    assert np.abs(m[..., 0].astype(np.float64) - 1.0).max() <= ld * EPS24 and (bits(m[..., 1:]) == 0).all()
