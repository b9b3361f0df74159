"""CPU: the attention-knockout additions to the C ABI, the bindings and the
façade's argument checks — no device is touched.
"""
import ctypes
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import tvr_amd
from tvr_amd import _lib, experiments

ROOT = Path(__file__).resolve().parents[1]
I32P, F32P, VP = r"const\s+int32_t\s*\*\s*", r"float\s*\*\s*", r"void\s*\*\s*"


def test_header_declares_and_library_exports_the_pieces():
    text = (ROOT / "include" / "tvr.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"TVR_SITE_ATTN_KNOCKOUT_LASTPOS\s*=\s*7\b", code)
    assert re.search(r"\bint\s+tvr_patch_sweep_knockout\s*\(\s*tvr_model\s*\*\s*model\s*,\s*tvr_trace\s*\*\s*trace\s*,"
                     r"\s*const\s+tvr_site\s*\*\s*sites\s*,\s*int32_t\s+n_sites\s*,\s*" + I32P + r"set_off\s*,\s*"
                     r"const\s+tvr_head_patch\s*\*\s*patches\s*,\s*" + I32P + r"key_off\s*,\s*" + I32P + r"keys\s*,\s*"
                     r"const\s+" + F32P + r"vectors\s*,\s*int32_t\s+n_vectors\s*,\s*" + F32P + r"out_prob\s*,\s*"
                     r"int32_t\s*\*\s*out_topk\s*,\s*int32_t\s+topk\s*,\s*" + F32P + r"out_logits\s*,\s*" + VP +
                     r"stream\s*\)", code)
    assert re.search(r"\bint\s+tvr_attention_knockout\s*\(\s*tvr_model\s*\*\s*model\s*,\s*int32_t\s+fmt\s*,\s*const\s+" +
                     F32P + r"qkv\s*,\s*const\s+" + F32P + r"cache\s*,\s*const\s+tvr_attn_seq\s*\*\s*seqs\s*,\s*"
                     r"int32_t\s+n_seq\s*,\s*int32_t\s+rows\s*,\s*int32_t\s+cache_rows\s*,\s*"
                     r"const\s+tvr_knockout_item\s*\*\s*items\s*,\s*int32_t\s+n_items\s*,\s*" + I32P + r"keys\s*,\s*"
                     r"int32_t\s+n_keys\s*,\s*" + VP + r"z\s*,\s*const\s+" + F32P + r"cos_t\s*,\s*const\s+" + F32P +
                     r"sin_t\s*,\s*" + VP + r"stream\s*\)", code)
    assert re.search(r"typedef\s+struct\s+tvr_knockout_item\s*\{\s*int32_t\s+seq\s*;\s*uint64_t\s+heads\s*;\s*int32_t\s+"
                     r"first_key\s*,\s*n_keys\s*;\s*\}", code)
    assert "#define TVR_ABI_VERSION 11" in text  # a backward-compatible addition
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(lib, "tvr_patch_sweep_knockout") and hasattr(lib, "tvr_attention_knockout")
    res, args = _lib.SIGNATURES["tvr_patch_sweep_knockout"]
    assert res is ctypes.c_int and len(args) == 15
    res, args = _lib.SIGNATURES["tvr_attention_knockout"]
    assert res is ctypes.c_int and len(args) == 16
    assert _lib.SITE_ATTN_KNOCKOUT_LASTPOS == 7
    assert _lib.load().tvr_abi_version() == _lib.ABI_VERSION == 11
    # seq @ 0, heads @ 8, first_key @ 16, n_keys @ 20: the C struct's natural layout
    K = _lib.CKnockoutItem
    assert ctypes.sizeof(K) == 24 and (K.seq.offset, K.heads.offset, K.first_key.offset, K.n_keys.offset) == (0, 8, 16, 20)
    assert _lib.KNOCKOUT_OPS == ("patch_sweep_knockout", "attention_knockout")
    assert _lib.SET_OPS == ("patch_sweep_sets",)
    assert ctypes.sizeof(_lib.CHbmStats) == 6 * (8 + 8 + 8) and len(_lib.HBM_KINDS) == 6  # timed under "attention"


def test_null_and_bad_arguments_are_invalid_without_a_device():
    lib = _lib.load()
    i32 = lambda *v: ctypes.cast((ctypes.c_int32 * len(v))(*v), ctypes.c_void_p)
    rc = lib.tvr_patch_sweep_knockout(None, None, None, 0, None, None, None, None, None, 0, None, None, 0, None, None)
    assert rc == _lib.TVR_ERR_INVALID and lib.tvr_last_error().startswith(b"tvr_patch_sweep_knockout: bad argument")
    fake = ctypes.cast((ctypes.c_char * 64)(), ctypes.c_void_p)  # never dereferenced: the offsets are checked first
    site = ctypes.cast((_lib.CSite * 1)(), ctypes.c_void_p)
    for set_off, key_off, patches, keys, msg in (
            (None, i32(0, 0), None, None, b"bad argument"),
            (i32(0, 0), None, None, None, b"bad argument"),
            (i32(-1, 0), i32(0, 0), None, None, b"set_off[0] is negative"),
            (i32(0, 0), i32(-1, 0), None, None, b"key_off[0] is negative"),
            (i32(1, 0), i32(0, 0), None, None, b"set_off decreases at site 0"),
            (i32(0, 0), i32(1, 0), None, None, b"key_off decreases at site 0"),
            (i32(0, 1), i32(0, 0), None, None, b"patches is null"),
            (i32(0, 0), i32(0, 1), None, None, b"keys is null")):
        rc = lib.tvr_patch_sweep_knockout(fake, fake, site, 1, set_off, patches, key_off, keys, None, 0, None, None, 0,
                                          None, None)
        assert rc == _lib.TVR_ERR_INVALID and msg in lib.tvr_last_error(), (msg, lib.tvr_last_error())
    rc = lib.tvr_attention_knockout(None, 0, None, None, None, 0, 0, 0, None, 0, None, 0, None, None, None, None)
    assert rc == _lib.TVR_ERR_INVALID and lib.tvr_last_error().startswith(b"tvr_attention_knockout: null model")
    # (everything behind a real model: tests/test_gpu_knockout.py)


def test_torch_op_schemas_and_host_checks():
    ops = _lib.load_ops()
    assert str(ops.patch_sweep_knockout.default._schema) == (
        "tvr::patch_sweep_knockout(int model, int trace, Tensor sites, Tensor set_off, Tensor patches, Tensor key_off, "
        "Tensor keys, Tensor? vectors, int topk, bool want_prob, bool want_logits, int d_vocab, Device device) "
        "-> (Tensor, Tensor, Tensor)")
    assert str(ops.attention_knockout.default._schema) == (
        "tvr::attention_knockout(int model, int fmt, Tensor qkv, Tensor? cache, Tensor seqs, Tensor items, Tensor keys, "
        "Tensor(a!) z, Tensor? cos_t, Tensor? sin_t) -> ()")
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)
    dev = torch.device("cpu")
    args = lambda **kw: [kw.get(k, v) for k, v in dict(
        model=1, trace=1, sites=i32(2, 9), set_off=i32(3), patches=i32(0, 3), key_off=i32(3), keys=i32(0), vectors=None,
        topk=0, want_prob=True, want_logits=False, d_vocab=8, device=dev).items()]
    for kw, msg in ((dict(sites=i32(2, 8)), r"sites must be \[n_sites, 9\]"),
                    (dict(sites=i32(0, 9), set_off=i32(1), key_off=i32(1)), "no patch sites"),
                    (dict(trace=0), "needs a trace"),
                    (dict(set_off=i32(2)), "set_off must be"),
                    (dict(key_off=i32(4)), "key_off must be"),
                    (dict(patches=i32(0, 2)), "patches must be"),
                    (dict(keys=i32(1, 1)), "keys must be"),
                    (dict(keys=torch.zeros(0)), "keys must be a contiguous CPU int32"),
                    (dict(set_off=torch.tensor([0, 1, 1], dtype=torch.int32)), "set_off runs past patches"),
                    (dict(key_off=torch.tensor([0, 0, 2], dtype=torch.int32)), "key_off runs past keys")):
        with pytest.raises(ValueError, match=msg):
            ops.patch_sweep_knockout(*args(**kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.patch_sweep_knockout(*args())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attention_knockout(1, 0, torch.zeros(4, 12), None, i32(1, 6), torch.zeros(1, 4, dtype=torch.int64), i32(0),
                               torch.zeros(4, 8), None, None)


def _host_model(n_layers=4, n_heads=4):
    cfg = tvr_amd.get_config("tiny").with_(n_layers=n_layers)
    m = types.SimpleNamespace(cfg=cfg, device=torch.device("cpu"), tokenizer=tvr_amd.tokenizer.SyntheticTokenizer(cfg.d_vocab))
    return m


def test_facade_value_errors_and_exports():
    m = _host_model()
    eff = experiments.attention_knockout_effect
    prompts, answers = [[0, 5, 6, 7], [0, 8, 9]], [3, 4]
    for kw, msg in ((dict(blocked=[[0, 1, 2, 3], []]), "every key"),
                    (dict(blocked=[[0], [0, 1, 2]]), "every key"),
                    (dict(blocked=[[4], []]), "outside the prompt"),
                    (dict(blocked=[[-1], []]), "outside the prompt"),
                    (dict(blocked=[[0]]), "one list of key positions per prompt"),
                    (dict(answers=[3]), "same length"),
                    (dict(windows=[(0, 4)]), "window"),
                    (dict(windows=[(2, 1)]), "window"),
                    (dict(windows=[(-1, 1)]), "window"),
                    (dict(heads=[0, 0]), "heads"),
                    (dict(heads=[4]), "heads"),
                    (dict(topk=0), "topk")):
        a = dict(blocked=[[0], [1]], windows=[(0, 1)], answers=answers, heads=None, topk=1)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            eff(prompts, a["answers"], a["blocked"], a["windows"], model=m, heads=a["heads"], topk=a["topk"])
    role = experiments.attention_knockout_by_role
    contexts = list(tvr_amd.tasks.letter_to_caps)
    for kw, msg in ((dict(num_contexts=0), "num_contexts"), (dict(len_contexts=len(contexts)), "len_contexts"),
                    (dict(roles=("bos", "nowhere")), "roles"), (dict(window=5), "window"), (dict(window=0), "window"),
                    (dict(stride=0), "window")):
        with pytest.raises(ValueError, match=msg):
            role(contexts, "→", ",", model=m, **kw)
    assert tvr_amd.attention_knockout_effect is eff and tvr_amd.attention_knockout_by_role is role
    assert hasattr(tvr_amd.Model, "patch_sweep_knockout")


def test_role_prompts_replay_the_sampler():
    """knockout_role_prompts returns sample_icl_prompts_with_roles' prompts and roles, the first label token of
    each query pair, and leaves the global random state where the sampler leaves it."""
    import random
    m = _host_model()
    contexts = list(tvr_amd.tasks.letter_to_caps)
    random.seed(5)
    want = tvr_amd.prompts.sample_icl_prompts_with_roles(m, contexts, "→", ",", 6, 3)
    after = random.random()
    random.seed(5)
    ps, roles, answers = experiments.knockout_role_prompts(m, contexts, "→", ",", 6, 3)
    assert (ps, roles) == want and random.random() == after
    enc = m.tokenizer.encode
    label = {tuple(enc(x)): enc(y)[0] for x, y in contexts}
    f = enc("→")
    for p, a in zip(ps, answers):
        assert p[-len(f):] == f
        query = next(k for k in label if tuple(p[-len(f) - len(k):-len(f)]) == k)
        assert a == label[query]
