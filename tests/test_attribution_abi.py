"""CPU: the logit-attribution and logit-lens pieces of the C ABI —
tvr_head_attribution, tvr_trace_logit_attribution, tvr_decode_rows and
tvr_trace_logit_lens — are declared, exported, bound and refuse null arguments
without a device; the torch operators have the documented schemas and host
checks; the façade checks its arguments before any engine call."""
import ctypes
import re
import types
from pathlib import Path

import pytest
import torch

import tvr_amd
from tvr_amd import _lib, experiments

ROOT = Path(__file__).resolve().parents[1]
I32P, CF32P, F32P, VP = r"const\s+int32_t\s*\*\s*", r"const\s+float\s*\*\s*", r"float\s*\*\s*", r"void\s*\*\s*"
I32 = r"int32_t\s+"
NAMES = ("tvr_head_attribution", "tvr_trace_logit_attribution", "tvr_decode_rows", "tvr_trace_logit_lens")


def test_header_declares_and_library_exports_the_pieces():
    text = (ROOT / "include" / "tvr.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    c = r"\s*,\s*"
    assert re.search(r"\bint\s+tvr_head_attribution\s*\(\s*tvr_model\s*\*\s*model" + c + I32 + "layer" + c + CF32P + "z" + c +
                     CF32P + "dirs" + c + I32 + "n" + c + F32P + "out" + c + VP + r"stream\s*\)", code)
    assert re.search(r"\bint\s+tvr_trace_logit_attribution\s*\(\s*tvr_trace\s*\*\s*trace" + c + I32P + "pos" + c + I32P +
                     "target" + c + I32P + "contrast" + c + F32P + "out_head" + c + F32P + "out_resid" + c + VP +
                     r"stream\s*\)", code)
    assert re.search(r"\bint\s+tvr_decode_rows\s*\(\s*tvr_model\s*\*\s*model" + c + CF32P + "rows" + c + I32 + "n" + c + I32P +
                     "targets" + c + F32P + "out_prob" + c + r"int32_t\s*\*\s*out_topk" + c + I32 + "topk" + c + VP +
                     r"stream\s*\)", code)
    assert re.search(r"\bint\s+tvr_trace_logit_lens\s*\(\s*tvr_trace\s*\*\s*trace" + c + I32P + "pos" + c + I32P + "targets" +
                     c + F32P + "out_prob" + c + r"int32_t\s*\*\s*out_topk" + c + I32 + "topk" + c + VP + r"stream\s*\)", code)
    assert "#define TVR_ABI_VERSION 11" in text  # backward-compatible additions
    assert re.search(r"TVR_HBM_KINDS\s*=\s*6\b", code)  # no new kind: the stats arrays are sized 6
    for name in NAMES:  # each is documented as an addition
        doc = text[:text.index("int " + name + "(")]
        assert "Backward-compatible addition: ABI 11" in doc[doc.rindex("/*"):], name
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, nargs in zip(NAMES, (7, 7, 8, 7)):
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    assert _lib.load().tvr_abi_version() == _lib.ABI_VERSION == 11
    assert ctypes.sizeof(_lib.CHbmStats) == 6 * (8 + 8 + 8) and len(_lib.HBM_KINDS) == 6
    assert _lib.ATTRIBUTION_OPS == ("head_attribution", "logit_attribution", "logit_lens", "decode_rows")
    assert _lib.STATS_MAX_K == 16
    # the earlier operator lists are unchanged
    assert _lib.OPS == ("forward_clean", "patch_sweep", "project_heads", "forward_logits")
    assert _lib.PATTERN_OPS == ("capture_pattern",) and _lib.RESID_OPS == ("capture_resid",)


def test_null_arguments_are_invalid_without_a_device():
    lib = _lib.load()
    buf = ctypes.cast((ctypes.c_float * 8)(), ctypes.c_void_p)
    ids = ctypes.cast((ctypes.c_int32 * 8)(), ctypes.c_void_p)

    def refused(rc, prefix):
        assert rc == _lib.TVR_ERR_INVALID and lib.tvr_last_error().startswith(prefix), (rc, lib.tvr_last_error())

    refused(lib.tvr_head_attribution(None, 0, buf, buf, 1, buf, None), b"tvr_head_attribution: null model")
    refused(lib.tvr_trace_logit_attribution(None, None, ids, None, buf, buf, None),
            b"tvr_trace_logit_attribution: null trace")
    refused(lib.tvr_decode_rows(None, buf, 1, ids, buf, None, 0, None), b"tvr_decode_rows: null model")
    refused(lib.tvr_trace_logit_lens(None, None, ids, buf, None, 0, None), b"tvr_trace_logit_lens: null trace")
    # (every refusal behind a real model or trace: tests/test_gpu_attribution.py)


def test_torch_op_schemas_and_host_checks():
    ops = _lib.load_ops()
    assert str(ops.head_attribution.default._schema) == (
        "tvr::head_attribution(int model, int layer, Tensor z, Tensor dirs, int d_model, int n_heads, Tensor(a!) out) -> ()")
    assert str(ops.logit_attribution.default._schema) == (
        "tvr::logit_attribution(int trace, Tensor? pos, Tensor target, Tensor? contrast, int n_seq, int n_layers, "
        "int n_heads, Tensor(a!)? out_head, Tensor(b!)? out_resid) -> ()")
    assert str(ops.logit_lens.default._schema) == (
        "tvr::logit_lens(int trace, Tensor? pos, Tensor? targets, int n_seq, int n_layers, int topk, "
        "Tensor(a!)? out_prob, Tensor(b!)? out_topk) -> ()")
    assert str(ops.decode_rows.default._schema) == (
        "tvr::decode_rows(int model, Tensor rows, Tensor? targets, int topk, int d_model, Tensor(a!)? out_prob, "
        "Tensor(b!)? out_topk) -> ()")
    # an existing schema, unchanged
    assert str(ops.capture_pattern.default._schema).startswith("tvr::capture_pattern(int trace, Tensor? pos, Tensor? cls,")
    i32 = lambda *a: torch.zeros(*a, dtype=torch.int32)  # noqa: E731
    heads, resid = torch.zeros(2, 3, 4), torch.zeros(2, 4)
    with pytest.raises(ValueError, match="needs a trace"):
        ops.logit_attribution(0, None, i32(2), None, 2, 3, 4, heads, resid)
    with pytest.raises(ValueError, match="out_head or out_resid"):
        ops.logit_attribution(1, None, i32(2), None, 2, 3, 4, None, None)
    with pytest.raises(ValueError, match="pos must have one entry"):
        ops.logit_attribution(1, i32(3), i32(2), None, 2, 3, 4, heads, resid)
    with pytest.raises(ValueError, match="target must have one entry"):
        ops.logit_attribution(1, None, i32(3), None, 2, 3, 4, heads, resid)
    with pytest.raises(ValueError, match="contrast must have one entry"):
        ops.logit_attribution(1, None, i32(2), i32(1), 2, 3, 4, heads, resid)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # CPU outputs: refused before the engine is called
        ops.logit_attribution(1, None, i32(2), None, 2, 3, 4, heads, resid)
    prob, top = torch.zeros(2, 4), i32(2, 4, 5)
    with pytest.raises(ValueError, match="needs a trace"):
        ops.logit_lens(0, None, i32(2), 2, 3, 0, prob, None)
    with pytest.raises(ValueError, match="out_prob or out_topk"):
        ops.logit_lens(1, None, i32(2), 2, 3, 0, None, None)
    with pytest.raises(ValueError, match="out_prob needs targets"):
        ops.logit_lens(1, None, None, 2, 3, 0, prob, None)
    with pytest.raises(ValueError, match="targets must have one entry"):
        ops.logit_lens(1, None, i32(3), 2, 3, 0, prob, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.logit_lens(1, None, i32(2), 2, 3, 5, prob, top)
    with pytest.raises(ValueError, match=r"rows must be \[n, d_model\]"):
        ops.decode_rows(1, torch.zeros(4), None, 1, 4, None, i32(1, 1))
    with pytest.raises(ValueError, match=r"rows must be \[n, d_model\]"):  # the width is the model's
        ops.decode_rows(1, torch.zeros(2, 4), None, 1, 8, None, i32(2, 1))
    with pytest.raises(ValueError, match="out_prob or out_topk"):
        ops.decode_rows(1, torch.zeros(2, 4), None, 1, 4, None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.decode_rows(1, torch.zeros(2, 4), i32(2), 0, 4, torch.zeros(2), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_attribution(1, 0, torch.zeros(2, 4), torch.zeros(2, 4), 4, 2, torch.zeros(2, 2))


def test_model_methods_check_their_arguments_on_the_host(tiny_cfg):
    """The checks run before the operator is reached (a stub stands in for the model: reaching ``_op`` would raise
    AttributeError)."""
    M = tvr_amd.Model

    def make_stub():
        st = types.SimpleNamespace(cfg=tiny_cfg, device=torch.device("cpu"), _check_topk=M._check_topk)
        for name in ("_trace_queries", "_token_ids"):  # the shared host checks
            setattr(st, name, types.MethodType(getattr(M, name), st))
        return st

    stub = make_stub()
    trace = types.SimpleNamespace(model=stub, seq_lens=[3, 2], _h=types.SimpleNamespace(value=1))
    V, d = tiny_cfg.d_vocab, tiny_cfg.d_model
    for fn, args in ((M.logit_attribution, ([1, 2],)), (M.logit_lens, ([1, 2],))):
        with pytest.raises(ValueError, match="another model"):
            fn(make_stub(), trace, *args)
        with pytest.raises(ValueError, match="trace is empty"):
            fn(stub, types.SimpleNamespace(model=stub, seq_lens=[]), *args)
        with pytest.raises(ValueError, match="one entry per traced sequence"):
            fn(stub, trace, *args, positions=[0])
        for pos in ([0, 2], [-1, 0], [3, 0]):
            with pytest.raises(ValueError, match="outside its sequence"):
                fn(stub, trace, *args, positions=pos)
        with pytest.raises(ValueError, match="one entry per row"):
            fn(stub, trace, [1])
        for bad in ([0, V], [-1, 0]):
            with pytest.raises(ValueError, match=r"outside \[0, d_vocab\)"):
                fn(stub, trace, bad)
    with pytest.raises(ValueError, match=r"contrast lies outside \[0, d_vocab\)"):
        M.logit_attribution(stub, trace, [1, 2], contrast=[0, V])
    with pytest.raises(AttributeError):  # accepted: the operator call follows
        M.logit_attribution(stub, trace, [1, 2], contrast=[3, 4], positions=[2, 0])
    for k in (-1, 17):
        with pytest.raises(ValueError, match="topk must be in"):
            M.logit_lens(stub, trace, [1, 2], topk=k)
        with pytest.raises(ValueError, match="topk must be in"):
            M.decode_rows(stub, torch.zeros(2, d), topk=k)
    with pytest.raises(ValueError, match="nothing to decode"):
        M.logit_lens(stub, trace)
    with pytest.raises(ValueError, match="nothing to decode"):
        M.decode_rows(stub, torch.zeros(2, d))
    for rows in (torch.zeros(d), torch.zeros(2, d + 1), torch.zeros(0, d), [[0.0] * d]):
        with pytest.raises(ValueError, match=r"rows must be a tensor \[n, d_model\]"):
            M.decode_rows(stub, rows, topk=1)
    with pytest.raises(ValueError, match="fp32 on the model device"):
        M.decode_rows(stub, torch.zeros(2, d, dtype=torch.float64), topk=1)
    with pytest.raises(ValueError, match="one entry per row"):
        M.decode_rows(stub, torch.zeros(2, d), targets=[1], topk=1)
    with pytest.raises(AttributeError):
        M.decode_rows(stub, torch.zeros(2, d), targets=[1, 2], topk=3)
    z = torch.zeros(3, d)
    for layer in (-1, tiny_cfg.n_layers):
        with pytest.raises(ValueError, match="layer out of range"):
            M.head_attribution(stub, layer, z, z)
    with pytest.raises(ValueError, match=r"dirs must be a tensor \[n, d_model\]"):
        M.head_attribution(stub, 0, z, torch.zeros(3, d - 1))
    with pytest.raises(ValueError, match="same number of rows"):
        M.head_attribution(stub, 0, z, torch.zeros(2, d))
    with pytest.raises(ValueError, match="fp32 on the model device"):
        M.head_attribution(stub, 0, z.double(), z)
    with pytest.raises(AttributeError):
        M.head_attribution(stub, 0, z, z)


def test_experiment_functions_check_their_arguments_before_any_engine_call(tiny_cfg):
    stub = types.SimpleNamespace(cfg=tiny_cfg)
    E = experiments
    assert tvr_amd.head_logit_attribution is E.head_logit_attribution
    assert tvr_amd.top_attribution_heads is E.top_attribution_heads
    assert tvr_amd.logit_lens_by_layer is E.logit_lens_by_layer and tvr_amd.decode_vectors is E.decode_vectors
    assert E.HeadLogitAttribution._fields == ("heads", "rest", "embed", "total")
    for fn in (E.head_logit_attribution, E.logit_lens_by_layer):
        with pytest.raises(ValueError, match="no prompts"):
            fn([], [], model=stub)
        with pytest.raises(ValueError, match="same length"):
            fn([[0, 1]], [1, 2], model=stub)
    with pytest.raises(ValueError, match="Contrast answers"):
        E.head_logit_attribution([[0, 1]], [1], model=stub, contrast_answers=[1, 2])
    for k in (0, 17):
        with pytest.raises(ValueError, match="topk must be in"):
            E.logit_lens_by_layer([[0, 1]], [1], model=stub, topk=k)
        with pytest.raises(ValueError, match="k must be in"):
            E.decode_vectors(torch.zeros(2, tiny_cfg.d_model), k, model=stub)
    with pytest.raises(ValueError, match="vectors must be of shape"):
        E.decode_vectors(torch.zeros(2, tiny_cfg.d_model + 1), 1, model=stub)
    with pytest.raises(AttributeError):  # accepted: the first engine access follows
        E.head_logit_attribution([[0, 1]], [[1]], model=stub)
    L, H = tiny_cfg.n_layers, tiny_cfg.n_heads
    heads = torch.zeros(L, H)
    heads[1, 2], heads[0, 1], heads[0, 3] = 0.9, 0.5, -2.0
    assert E.top_attribution_heads(heads, 2) == [(1, 2), (0, 1)]
    assert E.top_attribution_heads(heads, L * H)[-1] == (0, 3)
    for bad in (torch.zeros(L * H), [[0.0]]):
        with pytest.raises(ValueError, match="heads must be of shape"):
            E.top_attribution_heads(bad, 1)
    for k in (0, L * H + 1):
        with pytest.raises(ValueError, match="num_heads"):
            E.top_attribution_heads(heads, k)
