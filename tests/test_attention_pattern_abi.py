"""CPU: the attention-pattern pieces of the C ABI — tvr_attention_pattern,
tvr_trace_capture_pattern and the hooks TVR_TRACE_Q / _K / _V — are declared,
exported, bound and refuse null arguments without a device; the torch operator
has the documented schema and host checks; the role builders label every token
of their sibling prompt builder's prompt; the façade checks its arguments
before any engine call."""
import ctypes
import random
import re
import types
from pathlib import Path

import pytest
import torch

import tvr_amd
from tvr_amd import _lib, experiments, prompts
from tvr_amd.prompts import ROLES

ROOT = Path(__file__).resolve().parents[1]
I32P, F32P, VP = r"const\s+int32_t\s*\*\s*", r"float\s*\*\s*", r"void\s*\*\s*"


def test_header_declares_and_library_exports_the_pieces():
    text = (ROOT / "include" / "tvr.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+tvr_attention_pattern\s*\(\s*tvr_model\s*\*\s*model\s*,\s*const\s+" + F32P + r"qkv\s*,"
                     r"\s*int32_t\s+rows\s*,\s*" + I32P + r"row0\s*,\s*" + I32P + r"qpos\s*,\s*int32_t\s+n_seq\s*,\s*" +
                     I32P + r"cls\s*,\s*int32_t\s+n_classes\s*,\s*" + F32P + r"out_pattern\s*,\s*int32_t\s+ld\s*,\s*" +
                     F32P + r"out_mass\s*,\s*const\s+" + F32P + r"cos_t\s*,\s*const\s+" + F32P + r"sin_t\s*,\s*" + VP +
                     r"stream\s*\)", code)
    assert re.search(r"\bint\s+tvr_trace_capture_pattern\s*\(\s*tvr_trace\s*\*\s*trace\s*,\s*" + I32P + r"pos\s*,\s*" +
                     I32P + r"cls\s*,\s*int32_t\s+n_classes\s*,\s*" + F32P + r"out_pattern\s*,\s*int32_t\s+ld\s*,\s*" +
                     F32P + r"out_mass\s*,\s*" + VP + r"stream\s*\)", code)
    for name, value in (("Q", 2), ("K", 3), ("V", 4)):
        assert re.search(rf"TVR_TRACE_{name}\s*=\s*{value}\b", code)
    assert "#define TVR_ABI_VERSION 11" in text  # a backward-compatible addition
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(lib, "tvr_attention_pattern") and hasattr(lib, "tvr_trace_capture_pattern")
    res, args = _lib.SIGNATURES["tvr_attention_pattern"]
    assert res is ctypes.c_int and len(args) == 14
    res, args = _lib.SIGNATURES["tvr_trace_capture_pattern"]
    assert res is ctypes.c_int and len(args) == 8
    assert (_lib.TRACE_RESID_PRE, _lib.TRACE_Z, _lib.TRACE_Q, _lib.TRACE_K, _lib.TRACE_V) == (0, 1, 2, 3, 4)
    assert _lib.load().tvr_abi_version() == _lib.ABI_VERSION == 11
    # the stats record is part of the ABI: the capture is counted under the existing attention kind
    assert ctypes.sizeof(_lib.CHbmStats) == 6 * (8 + 8 + 8) and len(_lib.HBM_KINDS) == 6
    assert _lib.PATTERN_OPS == ("capture_pattern",)
    assert _lib.OPS == ("forward_clean", "patch_sweep", "project_heads", "forward_logits")
    assert _lib.SET_OPS == ("patch_sweep_sets",) and _lib.RESID_OPS == ("capture_resid",)


def test_null_arguments_are_invalid_without_a_device():
    lib = _lib.load()
    out = ctypes.cast((ctypes.c_float * 4)(), ctypes.c_void_p)
    rc = lib.tvr_trace_capture_pattern(None, None, None, 0, out, 4, None, None)
    assert rc == _lib.TVR_ERR_INVALID and lib.tvr_last_error().startswith(b"tvr_trace_capture_pattern: null trace")
    rc = lib.tvr_attention_pattern(None, None, 0, None, None, 0, None, 0, out, 4, None, None, None, None)
    assert rc == _lib.TVR_ERR_INVALID and lib.tvr_last_error().startswith(b"tvr_attention_pattern: null model")
    # (a null qkv behind a real model, and every other refusal: tests/test_gpu_attention_pattern.py)
    rc = lib.tvr_trace_read(None, _lib.TRACE_Q, 0, out, None)
    assert rc == _lib.TVR_ERR_INVALID and b"tvr_trace_read" in lib.tvr_last_error()


def test_torch_op_schema_and_host_checks():
    ops = _lib.load_ops()
    assert str(ops.capture_pattern.default._schema) == (
        "tvr::capture_pattern(int trace, Tensor? pos, Tensor? cls, int n_classes, int n_seq, int n_layers, "
        "int n_heads, Tensor(a!)? out_pattern, Tensor(b!)? out_mass) -> ()")
    pat, mass = torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 4, 7)
    cls = torch.zeros(9, dtype=torch.int32)
    with pytest.raises(ValueError, match="needs a trace"):
        ops.capture_pattern(0, None, None, 0, 2, 3, 4, pat, None)
    with pytest.raises(ValueError, match="out_pattern or out_mass"):
        ops.capture_pattern(1, None, None, 0, 2, 3, 4, None, None)
    with pytest.raises(ValueError, match="one entry per traced sequence"):
        ops.capture_pattern(1, torch.zeros(3, dtype=torch.int32), None, 0, 2, 3, 4, pat, None)
    with pytest.raises(ValueError, match="out_mass needs cls"):
        ops.capture_pattern(1, None, None, 7, 2, 3, 4, None, mass)
    with pytest.raises(ValueError, match="n_classes"):
        ops.capture_pattern(1, None, cls, 0, 2, 3, 4, pat, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # CPU outputs: refused before the engine is called
        ops.capture_pattern(1, None, cls, 7, 2, 3, 4, pat, mass)


class HostModel(tvr_amd.tokenizer.TokenizerMixin):
    """The token helpers alone (no engine): what the prompt builders use of a model."""
    device = "cpu"

    def __init__(self, vocab):
        self.tokenizer = tvr_amd.tokenizer.SyntheticTokenizer(vocab)


@pytest.fixture(scope="module")
def host_model(tiny_cfg):
    return HostModel(tiny_cfg.d_vocab)


def names(roles):
    return [ROLES[r] for r in roles]


def test_roles_label_every_token_of_the_sibling_prompt(host_model):
    assert ROLES == ("bos", "demo_input", "demo_function", "demo_label", "separator", "query_input", "self")
    single = list(tvr_amd.tasks.letter_to_caps)[:3]
    multi = [(" New Hampshire", " Concord"), (" Iowa", " Des Moines"), (" St. Paul", " Minnesota")]
    enc = host_model.tokenizer.encode
    assert len(enc(" New Hampshire")) == 2 and len(enc(" St. Paul")) == 3  # the items are multi-token
    for sep in (None, ","):
        ids = prompts.icl_single_token(host_model, single[:2], single[2][0], "→", sep)
        roles = prompts.icl_single_token_roles(host_model, single[:2], single[2][0], "→", sep)
        demo = ["demo_input", "demo_function", "demo_label"] + (["separator"] if sep else [])
        assert len(roles) == len(ids)
        assert names(roles) == ["bos"] + demo * 2 + (["separator"] if sep else []) + ["query_input", "self"]
        f = host_model.to_single_token("→")
        assert [i for i, r in zip(ids, roles) if ROLES[r] in ("demo_function", "self")] == [f] * 3
        if sep:  # the separator is doubled before the query
            assert names(roles)[-4:] == ["separator", "separator", "query_input", "self"]
            assert [i for i, r in zip(ids, roles) if ROLES[r] == "separator"] == [host_model.to_single_token(sep)] * 3

        for demos, query in ((multi[:2], multi[2][0]), (single[:2], single[2][0]), ([], multi[0][0])):
            ids = prompts.icl_multi_token(host_model, demos, query, "→", sep)
            roles = prompts.icl_multi_token_roles(host_model, demos, query, "→", sep)
            assert len(roles) == len(ids)
            want, at = ["bos"], 1
            for x, y in demos:
                want += ["demo_input"] * len(enc(x)) + ["demo_function"] + ["demo_label"] * len(enc(y))
                want += ["separator"] * (1 if sep else 0)
            want += ["separator"] * (1 if sep else 0) + ["query_input"] * len(enc(query)) + ["self"]
            assert names(roles) == want
            # each role's tokens are the sibling prompt's tokens of that item
            for x, y in demos:
                assert ids[at:at + len(enc(x))] == enc(x)
                at += len(enc(x)) + 1
                assert ids[at:at + len(enc(y))] == enc(y)
                at += len(enc(y)) + (1 if sep else 0)
    # a function token of two tokens: the last one is the query position, the one before belongs to the query
    roles = prompts.icl_multi_token_roles(host_model, multi[:1], multi[1][0], " is:", None)
    ids = prompts.icl_multi_token(host_model, multi[:1], multi[1][0], " is:", None)
    nf = len(enc(" is:"))
    assert nf == 2 and len(roles) == len(ids) and names(roles)[-1] == "self" and names(roles).count("self") == 1
    assert names(roles).count("demo_function") == nf and names(roles)[-2] == "query_input"
    with pytest.raises(AssertionError):  # as icl_single_token: every item must be one token
        prompts.icl_single_token_roles(host_model, multi[:1], multi[1][0], "→", None)


def test_sampling_with_roles_draws_as_sample_icl_prompts(host_model):
    contexts = list(tvr_amd.tasks.letter_to_caps)
    for sep in (None, ","):
        random.seed(11)
        want = prompts.sample_icl_prompts(host_model, contexts, "→", sep, 6, 3)
        state = random.getstate()
        random.seed(11)
        got, roles = prompts.sample_icl_prompts_with_roles(host_model, contexts, "→", sep, 6, 3)
        assert got == want and random.getstate() == state
        assert [len(r) for r in roles] == [len(p) for p in got]
        assert all(ROLES[r[-1]] == "self" and ROLES[r[0]] == "bos" for r in roles)
    assert contexts == list(tvr_amd.tasks.letter_to_caps)  # a private copy is shuffled


@pytest.fixture()
def stub_model(tiny_cfg):
    """Only ``cfg``: any engine or tokenizer call through it would raise AttributeError."""
    return types.SimpleNamespace(cfg=tiny_cfg)


def test_facade_argument_checks_raise_before_any_engine_call(stub_model, tiny_cfg):
    contexts = list(tvr_amd.tasks.letter_to_caps)
    prof = experiments.head_attention_profile
    with pytest.raises(ValueError, match="len_contexts"):
        prof(contexts[:4], "→", model=stub_model, num_contexts=8, len_contexts=4)
    with pytest.raises(ValueError, match="len_contexts"):
        prof(contexts[:4], "→", model=stub_model, num_contexts=8, len_contexts=-1)
    with pytest.raises(ValueError, match="num_contexts"):
        prof(contexts, "→", model=stub_model, num_contexts=0)
    with pytest.raises(AttributeError):  # accepted: the first tokenizer access follows
        prof(contexts[:5], "→", model=stub_model, num_contexts=1, len_contexts=4)
    assert tvr_amd.head_attention_profile is prof
    assert tvr_amd.top_attention_heads is experiments.top_attention_heads

    L, H = tiny_cfg.n_layers, tiny_cfg.n_heads
    profile = torch.zeros(L, H, len(ROLES))
    profile[1, 2, ROLES.index("demo_label")] = 0.9
    profile[0, 1, ROLES.index("demo_label")] = 0.5
    assert experiments.top_attention_heads(profile, "demo_label", 2) == [(1, 2), (0, 1)]
    assert experiments.top_attention_heads(profile, ROLES.index("demo_label"), 1) == [(1, 2)]
    for bad in (torch.zeros(L, H), torch.zeros(L, H, len(ROLES) + 1)):
        with pytest.raises(ValueError, match="profile must be of shape"):
            experiments.top_attention_heads(bad, "demo_label", 1)
    with pytest.raises(ValueError, match="role"):
        experiments.top_attention_heads(profile, "label", 1)
    with pytest.raises(ValueError, match="role"):
        experiments.top_attention_heads(profile, len(ROLES), 1)
    with pytest.raises(ValueError, match="num_heads"):
        experiments.top_attention_heads(profile, "demo_label", 0)
    with pytest.raises(ValueError, match="num_heads"):
        experiments.top_attention_heads(profile, "demo_label", L * H + 1)


def test_model_capture_pattern_checks_its_arguments_on_the_host(tiny_cfg):
    """Model.capture_pattern's checks run before the operator is reached (a stub stands in for the model:
    reaching ``_op`` would raise AttributeError)."""
    stub = types.SimpleNamespace(cfg=tiny_cfg, device="cpu")
    trace = types.SimpleNamespace(model=stub, seq_lens=[3, 2], _h=types.SimpleNamespace(value=1))
    cap = tvr_amd.Model.capture_pattern
    with pytest.raises(ValueError, match="another model"):
        cap(types.SimpleNamespace(cfg=tiny_cfg), trace, want_pattern=True)
    with pytest.raises(ValueError, match="trace is empty"):
        cap(stub, types.SimpleNamespace(model=stub, seq_lens=[]), want_pattern=True)
    with pytest.raises(ValueError, match="nothing to capture"):
        cap(stub, trace)
    with pytest.raises(ValueError, match="one entry per traced sequence"):
        cap(stub, trace, positions=[0], want_pattern=True)
    for pos in ([0, 2], [-1, 0], [3, 0]):
        with pytest.raises(ValueError, match="outside its sequence"):
            cap(stub, trace, positions=pos, want_pattern=True)
    for n_classes in (0, 65):
        with pytest.raises(ValueError, match="n_classes"):
            cap(stub, trace, classes=[0] * 5, n_classes=n_classes)
    for classes in ([0] * 4, [[0, 0, 0], [0]], [[0, 0], [0, 0, 0]]):
        with pytest.raises(ValueError, match="one entry per traced token"):
            cap(stub, trace, classes=classes, n_classes=2)
    for classes in ([0, 0, 2, 0, 0], [[0, -2, 0], [0, 0]]):
        with pytest.raises(ValueError, match=r"outside \[-1, n_classes\)"):
            cap(stub, trace, classes=classes, n_classes=2)
    with pytest.raises(AttributeError):  # accepted (flat and per sequence): the operator call follows
        cap(stub, trace, classes=[[0, -1, 1], [1, 0]], n_classes=2)
