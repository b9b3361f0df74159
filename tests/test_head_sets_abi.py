"""CPU: the joint head-set sweep's C ABI (tvr_patch_sweep_sets) is declared,
exported and validates its arguments before any device call; the experiment
façade checks its arguments before any engine call; head_ablation_curve's head
selection is assemble_task_vector's."""
import ctypes
import re
import types
from pathlib import Path

import pytest
import torch

import tvr_amd
from tvr_amd import _lib, experiments

ROOT = Path(__file__).resolve().parents[1]


def test_header_declares_and_library_exports_the_entry_point():
    text = (ROOT / "include" / "tvr.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+tvr_patch_sweep_sets\s*\(", code)
    assert re.search(r"TVR_SITE_REPLACE_HEADSET_ALLPOS\s*=\s*4\b", code)
    assert re.search(r"TVR_SITE_REPLACE_HEADSET_LASTPOS\s*=\s*5\b", code)
    body = re.search(r"typedef struct tvr_head_patch \{(.*?)\} tvr_head_patch;", code, re.S).group(1)
    assert re.findall(r"\w+", body.replace("int32_t", "")) == [f for f, _ in _lib.CHeadPatch._fields_]
    assert ctypes.sizeof(_lib.CHeadPatch) == 12
    assert "#define TVR_ABI_VERSION 11" in text  # a backward-compatible addition
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(lib, "tvr_patch_sweep_sets")
    assert "tvr_patch_sweep_sets" in _lib.SIGNATURES
    assert (_lib.SITE_REPLACE_HEADSET_ALLPOS, _lib.SITE_REPLACE_HEADSET_LASTPOS) == (4, 5)


def test_null_arguments_are_invalid_without_a_device():
    lib = _lib.load()
    rc = lib.tvr_patch_sweep_sets(None, None, None, 0, None, None, None, 0, None, None, 0, None, None)
    assert rc == _lib.TVR_ERR_INVALID
    assert b"tvr_patch_sweep_sets" in lib.tvr_last_error()
    # sites and offsets given, model / trace null: still rejected before anything is dereferenced
    sites = (_lib.CSite * 1)()
    off = (ctypes.c_int32 * 2)(0, 0)
    rc = lib.tvr_patch_sweep_sets(None, None, ctypes.cast(sites, ctypes.c_void_p), 1,
                                  ctypes.cast(off, ctypes.c_void_p), None, None, 0, None, None, 0, None, None)
    assert rc == _lib.TVR_ERR_INVALID


def test_torch_op_schema_and_host_checks():
    ops = _lib.load_ops()
    assert _lib.SET_OPS == ("patch_sweep_sets",)
    assert str(ops.patch_sweep_sets.default._schema) == (
        "tvr::patch_sweep_sets(int model, int trace, Tensor sites, Tensor set_off, Tensor patches, Tensor? vectors, "
        "int topk, bool want_prob, bool want_logits, int d_vocab, Device device) -> (Tensor, Tensor, Tensor)")
    dev = torch.device("cuda", 0)
    sites = torch.zeros(2, 9, dtype=torch.int32)
    i32 = dict(dtype=torch.int32)
    with pytest.raises(ValueError, match=r"\[n_sites \+ 1\]"):
        ops.patch_sweep_sets(1, 1, sites, torch.zeros(2, **i32), torch.zeros(0, 3, **i32), None, 0, True, False, 8, dev)
    with pytest.raises(ValueError, match=r"\[n_patches, 3\]"):
        ops.patch_sweep_sets(1, 1, sites, torch.zeros(3, **i32), torch.zeros(4, 2, **i32), None, 0, True, False, 8, dev)
    with pytest.raises(ValueError, match="runs past patches"):
        ops.patch_sweep_sets(1, 1, sites, torch.tensor([0, 1, 3], **i32), torch.zeros(2, 3, **i32), None, 0, True,
                             False, 8, dev)


@pytest.fixture()
def stub_model(tiny_cfg):
    """Only ``cfg``: any engine call through it would raise AttributeError."""
    return types.SimpleNamespace(cfg=tiny_cfg)


def test_facade_argument_checks_raise_before_any_engine_call(stub_model, tiny_cfg):
    L, H, d = tiny_cfg.n_layers, tiny_cfg.n_heads, tiny_cfg.d_model
    mean = torch.zeros(L, H, d)
    prompts, answers = [[0, 1, 2]], [3]
    jp = experiments.joint_head_patch_effect
    with pytest.raises(ValueError, match=r"Mean head activations must be of shape \(n_layers, n_heads, d_model\)"):
        jp(torch.zeros(L, H, d + 1), [[(0, 0)]], prompts, answers, model=stub_model)
    with pytest.raises(ValueError, match="Prompt answers must be of the same length as scrambled prompts"):
        jp(mean, [[(0, 0)]], prompts, [3, 4], model=stub_model)
    with pytest.raises(ValueError, match="positions"):
        jp(mean, [[(0, 0)]], prompts, answers, model=stub_model, positions="first")
    with pytest.raises(ValueError, match="out of range"):
        jp(mean, [[(L, 0)]], prompts, answers, model=stub_model)
    with pytest.raises(ValueError, match="twice"):
        jp(mean, [[(0, 1), (0, 1)]], prompts, answers, model=stub_model)
    hc = experiments.head_ablation_curve
    cie = torch.zeros(L, H)
    with pytest.raises(ValueError, match="count"):
        hc(mean, cie, prompts, answers, model=stub_model, counts=(L * H + 1,))
    with pytest.raises(ValueError, match="layer out of range"):
        hc(mean, cie, prompts, answers, model=stub_model, layer=L)
    with pytest.raises(ValueError, match="positions"):
        hc(mean, cie, prompts, answers, model=stub_model, counts=(1,), positions="middle")
    assert tvr_amd.joint_head_patch_effect is jp and tvr_amd.head_ablation_curve is hc


def test_head_selection_is_assemble_task_vectors(tiny_cfg):
    """A random CIE map with deliberate ties: the heads head_ablation_curve
    patches are the ones assemble_task_vector sums, in its order.  With one-hot
    'means' (mean[l, h] = e_{l*H+h}) the assembled vector is the indicator of
    the selected heads."""
    L, H = 5, tiny_cfg.n_heads
    g = torch.Generator().manual_seed(11)
    cie = torch.randint(0, 4, (L, H), generator=g).float() / 4  # 4 distinct values over L*H cells: many ties
    assert cie.unique().numel() < L * H
    mean = torch.eye(L * H).view(L, H, L * H)
    for layer in (0, 2, L - 1):
        for k in (1, 2, 5, H * (layer + 1)):
            if k > H * (layer + 1):
                continue
            heads = experiments.top_cie_heads(cie, layer, k)
            assert len(heads) == k == len(set(heads)) and all(l <= layer for l, _ in heads)
            vec = experiments.assemble_task_vector(mean, cie, layer, k)
            want = torch.zeros(L * H)
            want[[l * H + h for l, h in heads]] = 1
            assert torch.equal(vec, want)
            _, idx = torch.topk(cie[: layer + 1].flatten(), k)  # the reference's own selection
            assert heads == [(int(i) // H, int(i) % H) for i in idx]


def test_curve_head_lists_and_controls(monkeypatch, stub_model, tiny_cfg):
    """head_ablation_curve hands joint_head_patch_effect the top-k lists
    (assemble_task_vector's selection) followed by the seeded control sets."""
    import random
    L, H, d = tiny_cfg.n_layers, tiny_cfg.n_heads, tiny_cfg.d_model
    g = torch.Generator().manual_seed(5)
    cie = torch.randint(0, 3, (L, H), generator=g).float()
    seen = {}

    def fake(mean, sets, prompts, answers, model=None, positions="all", topk=1):
        seen["sets"], seen["positions"] = sets, positions
        n = len(sets)
        return {"dprob": torch.arange(n).float(), "accuracy": torch.zeros(n), "clean_prob": 0.5, "clean_accuracy": 1.0}

    monkeypatch.setattr(experiments, "joint_head_patch_effect", fake)
    counts, layer = (1, 2, 3), L - 2
    r = experiments.head_ablation_curve(torch.zeros(L, H, d), cie, [[0, 1]], [2], model=stub_model, counts=counts,
                                        layer=layer, n_random=2, seed=7, positions="last")
    tops = [experiments.top_cie_heads(cie, layer, k) for k in counts]
    rng = random.Random(7)
    pool = [(l, h) for l in range(layer + 1) for h in range(H)]
    ctrl = [[rng.sample(pool, k) for _ in range(2)] for k in counts]
    assert r["heads"] == tops and r["random_heads"] == ctrl and r["counts"] == list(counts)
    assert seen["sets"] == tops + [s for per_k in ctrl for s in per_k] and seen["positions"] == "last"
    assert r["top"]["dprob"].tolist() == [0.0, 1.0, 2.0]
    assert r["random"]["dprob"].tolist() == [[3.0, 4.0], [5.0, 6.0], [7.0, 8.0]]
