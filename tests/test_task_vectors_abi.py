"""CPU: the residual-stream task-vector pieces of the C ABI — the grouped
capture tvr_trace_capture_resid and the site kind TVR_SITE_SET_RESID_PRE_VEC —
are declared, exported, bound and validate their arguments before any device
call; the experiment façade checks its arguments before any engine call."""
import ctypes
import re
import types
from pathlib import Path

import pytest
import torch

import tvr_amd
from tvr_amd import _lib, experiments

ROOT = Path(__file__).resolve().parents[1]


def test_header_declares_and_library_exports_the_pieces():
    text = (ROOT / "include" / "tvr.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+tvr_trace_capture_resid\s*\(\s*tvr_trace\s*\*\s*trace\s*,\s*const\s+int32_t\s*\*\s*pos\s*,"
                     r"\s*const\s+int32_t\s*\*\s*group\s*,\s*int32_t\s+n_groups\s*,\s*float\s*\*\s*out\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", code)
    assert re.search(r"TVR_SITE_SET_RESID_PRE_VEC\s*=\s*6\b", code)
    assert "#define TVR_ABI_VERSION 11" in text  # a backward-compatible addition
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(lib, "tvr_trace_capture_resid")
    res, args = _lib.SIGNATURES["tvr_trace_capture_resid"]
    assert res is ctypes.c_int and len(args) == 6
    assert _lib.SITE_SET_RESID_PRE_VEC == 6
    assert _lib.load().tvr_abi_version() == _lib.ABI_VERSION == 11
    # the stats record is part of the ABI: the capture is counted under the existing kind, no new slot
    assert ctypes.sizeof(_lib.CHbmStats) == 6 * (8 + 8 + 8) and len(_lib.HBM_KINDS) == 6


def test_null_arguments_are_invalid_without_a_device():
    lib = _lib.load()
    rc = lib.tvr_trace_capture_resid(None, None, None, 0, None, None)
    assert rc == _lib.TVR_ERR_INVALID
    assert b"tvr_trace_capture_resid" in lib.tvr_last_error()
    out = (ctypes.c_float * 4)()  # an output alone does not help: the trace is still null
    rc = lib.tvr_trace_capture_resid(None, None, None, 1, ctypes.cast(out, ctypes.c_void_p), None)
    assert rc == _lib.TVR_ERR_INVALID
    assert b"tvr_trace_capture_resid" in lib.tvr_last_error()


def test_torch_op_schema_and_host_checks():
    ops = _lib.load_ops()
    assert _lib.RESID_OPS == ("capture_resid",)
    assert _lib.OPS == ("forward_clean", "patch_sweep", "project_heads", "forward_logits")
    assert _lib.SET_OPS == ("patch_sweep_sets",)
    assert str(ops.capture_resid.default._schema) == (
        "tvr::capture_resid(int trace, Tensor? pos, Tensor? groups, int n_groups, int n_seq, Tensor(a!) out) "
        "-> Tensor(a!)")
    out = torch.zeros(1, 3, 8)
    with pytest.raises(ValueError, match="needs a trace"):
        ops.capture_resid(0, None, None, 1, 2, out)
    with pytest.raises(ValueError, match="n_groups"):
        ops.capture_resid(1, None, None, 0, 2, out)
    with pytest.raises(ValueError, match="one entry per traced sequence"):
        ops.capture_resid(1, torch.zeros(3, dtype=torch.int32), None, 1, 2, out)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a CPU output: refused before the engine is called
        ops.capture_resid(1, None, None, 1, 2, out)


@pytest.fixture()
def stub_model(tiny_cfg):
    """Only ``cfg``: any engine or tokenizer call through it would raise AttributeError."""
    return types.SimpleNamespace(cfg=tiny_cfg)


def test_facade_argument_checks_raise_before_any_engine_call(stub_model, tiny_cfg):
    L, d = tiny_cfg.n_layers, tiny_cfg.d_model
    contexts = list(tvr_amd.tasks.letter_to_caps)
    for fn in (experiments.apply_task_vectors_to_zero_shot, experiments.apply_task_vectors_to_zero_shot_by_probability):
        for bad in (torch.zeros(L + 2, d), torch.zeros(L - 1, d), torch.zeros(L, d + 1), torch.zeros(L, 1, d),
                    torch.zeros(d)):
            with pytest.raises(ValueError, match=r"task_vectors must be of shape"):
                fn(bad, contexts, "→", model=stub_model)
        for ok in (torch.zeros(L, d), torch.zeros(L + 1, d)):  # accepted: the first engine-side access follows
            with pytest.raises(AttributeError):
                fn(ok, contexts, "→", model=stub_model)
    ex = experiments.extract_task_vectors
    with pytest.raises(ValueError, match="len_contexts"):
        ex(contexts[:4], "→", stub_model, num_contexts=8, len_contexts=4)
    with pytest.raises(ValueError, match="len_contexts"):
        ex(contexts[:4], "→", stub_model, num_contexts=8, len_contexts=7)
    with pytest.raises(ValueError, match="num_contexts"):
        ex(contexts, "→", stub_model, num_contexts=0)
    with pytest.raises(AttributeError):  # len_contexts = len(contexts) - 1 is the largest that leaves a query
        ex(contexts[:5], "→", stub_model, num_contexts=1, len_contexts=4)
    assert tvr_amd.extract_task_vectors is ex
    assert tvr_amd.apply_task_vectors_to_zero_shot is experiments.apply_task_vectors_to_zero_shot
    assert tvr_amd.apply_task_vectors_to_zero_shot_by_probability is \
        experiments.apply_task_vectors_to_zero_shot_by_probability


def test_site_helpers_keep_their_default_kind():
    """The vector-site helpers were generalised by a ``kind`` argument; the
    existing callers (no argument) still build ADD_ATTN_OUT_LASTPOS sites."""
    import inspect
    for fn in (experiments._add_site_outputs, experiments._injection_sweep, experiments._zero_shot_accuracy,
               experiments._zero_shot_dprob):
        assert inspect.signature(fn).parameters["kind"].default == _lib.SITE_ADD_ATTN_OUT_LASTPOS
