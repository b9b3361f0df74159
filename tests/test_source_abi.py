"""CPU: the per-source-token attribution pieces of the C ABI — tvr_head_directions,
tvr_attention_source and tvr_trace_source_attribution — are declared, exported,
bound and refuse null arguments without a device; the torch operators have the
documented schemas and host checks; the façade checks its arguments before any
engine call."""
import ctypes
import re
import types
from pathlib import Path

import pytest
import torch

import tvr_amd
from tvr_amd import _lib, experiments
from tvr_amd.prompts import ROLES

ROOT = Path(__file__).resolve().parents[1]
I32P, CF32P, F32P, VP = r"const\s+int32_t\s*\*\s*", r"const\s+float\s*\*\s*", r"float\s*\*\s*", r"void\s*\*\s*"
I32 = r"int32_t\s+"
NAMES = ("tvr_head_directions", "tvr_attention_source", "tvr_trace_source_attribution")


def test_header_declares_and_library_exports_the_pieces():
    text = (ROOT / "include" / "tvr.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    c = r"\s*,\s*"
    assert re.search(r"\bint\s+tvr_head_directions\s*\(\s*tvr_model\s*\*\s*model" + c + I32 + "layer" + c + CF32P + "dirs" + c +
                     I32 + "n" + c + F32P + "out_g" + c + VP + r"stream\s*\)", code)
    assert re.search(r"\bint\s+tvr_attention_source\s*\(\s*tvr_model\s*\*\s*model" + c + CF32P + "qkv" + c + I32 + "rows" + c +
                     I32P + "row0" + c + I32P + "qpos" + c + I32 + "n_seq" + c + CF32P + "g" + c + I32P + "cls" + c + I32 +
                     "n_classes" + c + F32P + "out_src" + c + I32 + "ld" + c + F32P + "out_cls" + c + CF32P + "cos_t" + c +
                     CF32P + "sin_t" + c + VP + r"stream\s*\)", code)
    assert re.search(r"\bint\s+tvr_trace_source_attribution\s*\(\s*tvr_trace\s*\*\s*trace" + c + I32P + "pos" + c + I32P +
                     "target" + c + I32P + "contrast" + c + I32P + "cls" + c + I32 + "n_classes" + c + F32P + "out_src" + c +
                     I32 + "ld" + c + F32P + "out_cls" + c + VP + r"stream\s*\)", code)
    assert "#define TVR_ABI_VERSION 11" in text  # backward-compatible additions
    assert re.search(r"TVR_HBM_KINDS\s*=\s*6\b", code)  # no new kind: the stats arrays are sized 6
    for name in NAMES:  # each is documented as an addition
        doc = text[:text.index("int " + name + "(")]
        assert "Backward-compatible addition: ABI 11" in doc[doc.rindex("/*"):], name
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, nargs in zip(NAMES, (6, 15, 10)):
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    assert _lib.load().tvr_abi_version() == _lib.ABI_VERSION == 11
    assert ctypes.sizeof(_lib.CHbmStats) == 6 * (8 + 8 + 8) and len(_lib.HBM_KINDS) == 6
    assert _lib.SOURCE_OPS == ("head_directions", "attention_source", "source_attribution")
    # the earlier operator lists are unchanged
    assert _lib.OPS == ("forward_clean", "patch_sweep", "project_heads", "forward_logits")
    assert _lib.SET_OPS == ("patch_sweep_sets",) and _lib.KNOCKOUT_OPS == ("patch_sweep_knockout", "attention_knockout")
    assert _lib.PATTERN_OPS == ("capture_pattern",) and _lib.RESID_OPS == ("capture_resid",)
    assert _lib.ATTRIBUTION_OPS == ("head_attribution", "logit_attribution", "logit_lens", "decode_rows")
    assert _lib.PATTERN_MAX_CLASSES == 64


def test_null_arguments_are_invalid_without_a_device():
    lib = _lib.load()
    buf = ctypes.cast((ctypes.c_float * 8)(), ctypes.c_void_p)
    ids = ctypes.cast((ctypes.c_int32 * 8)(), ctypes.c_void_p)

    def refused(rc, prefix):
        assert rc == _lib.TVR_ERR_INVALID and lib.tvr_last_error().startswith(prefix), (rc, lib.tvr_last_error())

    refused(lib.tvr_head_directions(None, 0, buf, 1, buf, None), b"tvr_head_directions: null model")
    refused(lib.tvr_attention_source(None, buf, 1, ids, ids, 1, buf, None, 0, buf, 1, None, None, None, None),
            b"tvr_attention_source: null model")
    refused(lib.tvr_trace_source_attribution(None, None, ids, None, None, 0, buf, 1, None, None),
            b"tvr_trace_source_attribution: null trace")
    # (every refusal behind a real model or trace: tests/test_gpu_source_attribution.py)


def test_torch_op_schemas_and_host_checks():
    ops = _lib.load_ops()
    for name in _lib.SOURCE_OPS:
        assert hasattr(ops, name)
    assert str(ops.head_directions.default._schema) == (
        "tvr::head_directions(int model, int layer, Tensor dirs, int d_model, Tensor(a!) out_g) -> ()")
    assert str(ops.attention_source.default._schema) == (
        "tvr::attention_source(int model, Tensor qkv, Tensor row0, Tensor qpos, Tensor g, Tensor? cls, int n_classes, "
        "int d_model, int n_heads, Tensor(a!)? out_src, Tensor(b!)? out_cls, Tensor? cos_t, Tensor? sin_t) -> ()")
    assert str(ops.source_attribution.default._schema) == (
        "tvr::source_attribution(int trace, Tensor? pos, Tensor target, Tensor? contrast, Tensor? cls, int n_classes, "
        "int n_seq, int n_layers, int n_heads, Tensor(a!)? out_src, Tensor(b!)? out_cls) -> ()")
    # existing schemas, unchanged
    assert str(ops.capture_pattern.default._schema).startswith("tvr::capture_pattern(int trace, Tensor? pos, Tensor? cls,")
    assert str(ops.logit_attribution.default._schema).startswith("tvr::logit_attribution(int trace, Tensor? pos, Tensor target,")
    i32 = lambda *a: torch.zeros(*a, dtype=torch.int32)  # noqa: E731
    src, cls_out = torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 4, 6)
    with pytest.raises(ValueError, match="needs a trace"):
        ops.source_attribution(0, None, i32(2), None, None, 0, 2, 3, 4, src, None)
    with pytest.raises(ValueError, match="out_src or out_cls"):
        ops.source_attribution(1, None, i32(2), None, None, 0, 2, 3, 4, None, None)
    with pytest.raises(ValueError, match="pos must have one entry"):
        ops.source_attribution(1, i32(3), i32(2), None, None, 0, 2, 3, 4, src, None)
    with pytest.raises(ValueError, match="target must have one entry"):
        ops.source_attribution(1, None, i32(3), None, None, 0, 2, 3, 4, src, None)
    with pytest.raises(ValueError, match="contrast must have one entry"):
        ops.source_attribution(1, None, i32(2), i32(1), None, 0, 2, 3, 4, src, None)
    with pytest.raises(ValueError, match="out_cls needs cls"):
        ops.source_attribution(1, None, i32(2), None, None, 6, 2, 3, 4, src, cls_out)
    with pytest.raises(ValueError, match="n_classes must be positive"):
        ops.source_attribution(1, None, i32(2), None, i32(9), 0, 2, 3, 4, src, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # CPU outputs: refused before the engine is called
        ops.source_attribution(1, None, i32(2), None, i32(9), 6, 2, 3, 4, src, cls_out)
    qkv, g = torch.zeros(7, 24), torch.zeros(2, 8)
    with pytest.raises(ValueError, match="out_src or out_cls"):
        ops.attention_source(1, qkv, i32(2), i32(2), g, None, 0, 8, 2, None, None, None, None)
    with pytest.raises(ValueError, match="out_cls needs cls"):
        ops.attention_source(1, qkv, i32(2), i32(2), g, None, 3, 8, 2, None, torch.zeros(2, 2, 3), None, None)
    with pytest.raises(ValueError, match="one entry per sequence"):
        ops.attention_source(1, qkv, i32(2), i32(3), g, None, 0, 8, 2, torch.zeros(2, 2, 5), None, None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attention_source(1, qkv, i32(2), i32(2), g, None, 0, 8, 2, torch.zeros(2, 2, 5), None, None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_directions(1, 0, torch.zeros(2, 8), 8, torch.zeros(2, 8))


def test_model_methods_check_their_arguments_on_the_host(tiny_cfg):
    """The checks run before the operator is reached (a stub stands in for the model: reaching ``_op`` would raise
    AttributeError)."""
    M = tvr_amd.Model

    def make_stub():
        st = types.SimpleNamespace(cfg=tiny_cfg, device=torch.device("cpu"))
        for name in ("_trace_queries", "_token_ids"):  # the shared host checks
            setattr(st, name, types.MethodType(getattr(M, name), st))
        return st

    stub = make_stub()
    trace = types.SimpleNamespace(model=stub, seq_lens=[3, 2], _h=types.SimpleNamespace(value=1))
    V, d = tiny_cfg.d_vocab, tiny_cfg.d_model
    fn = M.source_attribution
    with pytest.raises(ValueError, match="another model"):
        fn(make_stub(), trace, [1, 2], want_keys=True)
    with pytest.raises(ValueError, match="trace is empty"):
        fn(stub, types.SimpleNamespace(model=stub, seq_lens=[]), [1, 2], want_keys=True)
    with pytest.raises(ValueError, match="one entry per traced sequence"):
        fn(stub, trace, [1, 2], positions=[0], want_keys=True)
    for pos in ([0, 2], [-1, 0], [3, 0]):
        with pytest.raises(ValueError, match="outside its sequence"):
            fn(stub, trace, [1, 2], positions=pos, want_keys=True)
    with pytest.raises(ValueError, match="one entry per row"):
        fn(stub, trace, [1], want_keys=True)
    for bad in ([0, V], [-1, 0]):
        with pytest.raises(ValueError, match=r"outside \[0, d_vocab\)"):
            fn(stub, trace, bad, want_keys=True)
    with pytest.raises(ValueError, match=r"contrast lies outside \[0, d_vocab\)"):
        fn(stub, trace, [1, 2], contrast=[0, V], want_keys=True)
    with pytest.raises(ValueError, match="nothing to attribute"):
        fn(stub, trace, [1, 2])
    for k in (0, 65):
        with pytest.raises(ValueError, match=r"n_classes must be in \[1, 64\]"):
            fn(stub, trace, [1, 2], classes=[0] * 5, n_classes=k)
    with pytest.raises(ValueError, match="one entry per traced token"):
        fn(stub, trace, [1, 2], classes=[0] * 4, n_classes=2)
    with pytest.raises(ValueError, match="one entry per traced token"):
        fn(stub, trace, [1, 2], classes=[[0, 0], [0, 0]], n_classes=2)
    for bad in ([0, 0, 2, 0, 0], [0, -2, 0, 0, 0]):
        with pytest.raises(ValueError, match=r"outside \[-1, n_classes\)"):
            fn(stub, trace, [1, 2], classes=bad, n_classes=2)
    with pytest.raises(AttributeError):  # accepted: the operator call follows
        fn(stub, trace, [1, 2], contrast=[3, 4], positions=[2, 0], classes=[[0, 1, -1], [1, 0]], n_classes=2)
    with pytest.raises(AttributeError):
        fn(stub, trace, [1, 2], want_keys=True)
    dirs = torch.zeros(3, d)
    for layer in (-1, tiny_cfg.n_layers):
        with pytest.raises(ValueError, match="layer out of range"):
            M.head_directions(stub, layer, dirs)
    for bad in (torch.zeros(d), torch.zeros(3, d - 1), torch.zeros(0, d), [[0.0] * d]):
        with pytest.raises(ValueError, match=r"dirs must be a tensor \[n, d_model\]"):
            M.head_directions(stub, 0, bad)
    with pytest.raises(ValueError, match="fp32 on the model device"):
        M.head_directions(stub, 0, dirs.double())
    with pytest.raises(AttributeError):
        M.head_directions(stub, 0, dirs)
    # Trace.source_attribution forwards every argument
    seen = {}
    tr = types.SimpleNamespace(model=types.SimpleNamespace(source_attribution=lambda t, tg, **kw: seen.update(kw, tg=tg)))
    tvr_amd.Trace.source_attribution(tr, [1], contrast=[2], pos=[0], classes=[0], n_classes=1, want_keys=True)
    assert seen == dict(tg=[1], contrast=[2], positions=[0], classes=[0], n_classes=1, want_keys=True)


def test_experiment_functions_check_their_arguments_before_any_engine_call(tiny_cfg):
    stub = types.SimpleNamespace(cfg=tiny_cfg)
    E = experiments
    assert tvr_amd.head_source_attribution is E.head_source_attribution
    assert tvr_amd.top_source_heads is E.top_source_heads
    contexts = [("a", "A"), ("b", "B"), ("c", "C")]
    with pytest.raises(ValueError, match="num_contexts must be positive"):
        E.head_source_attribution(contexts, "→", model=stub, num_contexts=0)
    for n in (-1, 3):
        with pytest.raises(ValueError, match="len_contexts must be smaller"):
            E.head_source_attribution(contexts, "→", model=stub, num_contexts=2, len_contexts=n)
    with pytest.raises(ValueError, match="Contrast answers"):
        E.head_source_attribution(contexts, "→", model=stub, num_contexts=2, len_contexts=2, contrast_answers=[1])
    with pytest.raises(AttributeError):  # accepted: the first engine access (the tokenizer) follows
        E.head_source_attribution(contexts, "→", model=stub, num_contexts=2, len_contexts=2, contrast_answers=[1, 2])
    L, H, R = tiny_cfg.n_layers, tiny_cfg.n_heads, len(ROLES)
    prof = torch.zeros(L, H, R)
    role = ROLES.index("demo_label")
    prof[1, 2, role], prof[0, 1, role], prof[0, 3, role] = 0.9, 0.5, -2.0  # (an attribution may be negative)
    prof[0, 0, 0] = 5.0  # another role's column does not count
    assert E.top_source_heads(prof, "demo_label", 2) == [(1, 2), (0, 1)]
    assert E.top_source_heads(prof, role, 2) == [(1, 2), (0, 1)]
    assert E.top_source_heads(prof, role, L * H)[-1] == (0, 3)
    assert E.top_source_heads(prof, 0, 1) == [(0, 0)]
    for bad in (torch.zeros(L, H), torch.zeros(L, H, R + 1), [[0.0]]):
        with pytest.raises(ValueError, match="profile must be of shape"):
            E.top_source_heads(bad, role, 1)
    with pytest.raises(ValueError, match="role must be one of"):
        E.top_source_heads(prof, "no_such_role", 1)
    with pytest.raises(ValueError, match="role must be one of"):
        E.top_source_heads(prof, R, 1)
    for k in (0, L * H + 1):
        with pytest.raises(ValueError, match="num_heads"):
            E.top_source_heads(prof, role, k)
