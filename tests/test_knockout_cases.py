"""CPU: the knockout references of knockout_cases.py against the oracle, and the
negative control of tests/test_gpu_knockout.py's end-to-end cases.

* the hooked recomputation with nothing blocked reproduces ``hook_z`` (1e-12, fp64);
* with blocked keys it equals an independently written full forward whose scores
  are ``masked_fill``'ed (1e-12), the knocked pattern sums to 1 and is 0 on B;
* the primitive's fp64 reference equals its two fp32 restatements to their bar
  by construction — here the three forms are held together in fp64 (1e-12);
* every end-to-end case moves the fp64 last-position logits by more than 100 x
  the logit bar the GPU test holds the engine to: an engine that ignored the
  knockout would fail there.
"""
import numpy as np
import pytest
import torch

import attention_cases as A
import knockout_cases as K
import tvr_amd
from conftest import make_oracle


class HostModel(tvr_amd.tokenizer.TokenizerMixin):
    """The token helpers alone (no engine): what the prompt builders use of a model."""
    device = "cpu"

    def __init__(self, vocab):
        self.tokenizer = tvr_amd.tokenizer.SyntheticTokenizer(vocab)


@pytest.fixture(scope="module")
def tiny4():
    cfg = tvr_amd.get_config("tiny").with_(n_layers=4)
    sd = tvr_amd.weights.synth_hf_state_dict(cfg, seed=0, std=0.15)
    tok = tvr_amd.tokenizer.SyntheticTokenizer(cfg.d_vocab)
    return cfg, make_oracle(cfg, sd, tok, torch.float64)


def test_nothing_blocked_reproduces_hook_z(tiny4):
    cfg, o64 = tiny4
    for p in K.e2e_prompts(cfg):
        _, cache = o64.run_with_cache(torch.tensor([p]))
        for l in range(cfg.n_layers):
            z, pat = K.knocked_z(o64, l, cache[f"blocks.{l}.hook_resid_pre"], range(cfg.n_heads), [])
            for h in range(cfg.n_heads):
                assert (z[h] - cache[f"blocks.{l}.attn.hook_z"][0, -1, h]).abs().max() < 1e-12
                assert abs(pat[h].sum().item() - 1) < 1e-12


def test_hooked_knockout_equals_a_masked_forward(tiny4):
    cfg, o64 = tiny4
    for p in K.e2e_prompts(cfg):
        clean = o64(torch.tensor([p]))[0, -1]
        assert (K.knocked_logits(o64, p, [(0, 0)], []) - clean).abs().max() == 0
        for members, keys in K.e2e_cases(cfg, len(p)):
            a = K.knocked_logits(o64, p, members, keys)
            b = K.masked_forward_logits(o64, p, members, keys)
            assert (a - b).abs().max() < 1e-12 * max(1.0, b.abs().max().item()), (len(p), members, keys)
            # the pattern of the first member at its layer: sums to 1, zero on the blocked keys
            l, h = members[0]
            _, cache = o64.run_with_cache(torch.tensor([p]))
            if l == min(m[0] for m in members):  # (its residual is still the clean one)
                _, pat = K.knocked_z(o64, l, cache[f"blocks.{l}.hook_resid_pre"], [h], keys)
                assert abs(pat[h].sum().item() - 1) < 1e-12 and (pat[h][keys] == 0).all()
                assert (pat[h] >= 0).all()


@pytest.mark.parametrize("model", [(16, 6), (80, 4), (128, 3)], ids=lambda m: f"dh{m[0]}h{m[1]}")
def test_the_three_forms_agree_in_fp64(model):
    cos, sin = A.tables(model[0], dtype=torch.float64)
    for T in (2, 17, 65):
        case = K.make(model, T)
        for fam in K.FAMILIES:
            items = K.items_of(case, fam, cos, sin)
            if not items:
                continue
            z = K.reference(case, items, cos, sin)
            for form in ("plain", "online"):
                other = K._knocked(case, items, cos, sin, torch.float64, form)[0]
                assert np.abs(other - z).max() < 1e-12 * max(1.0, np.abs(z).max()), (T, fam, form)
            for it, p in zip(items, K.pattern64(case, items, cos, sin)):
                assert abs(p.sum().item() - 1) < 1e-12 and (p[list(it.keys)] == 0).all()
            b, e1, e2 = K.bar(case, items, cos.astype(np.float32), sin.astype(np.float32), None)
            assert max(e1, e2) <= b and 0 < b < 1e-4 * case.max_v()  # (all_but_one: one key, both errors 0)


def test_select_cases_are_exact_in_fp32():
    """The restatements of a select case return the runner-up's V row bit for bit."""
    for model in K.MODELS:
        cos, sin = A.tables(model[0])
        for T in (15, 33, 65):
            case, items, expect = K.make_select(model, T)
            for f in (K.restate_plain, K.restate_online):
                assert np.array_equal(f(case, items, cos, sin), expect), (model, T, f.__name__)


def test_families_exist_where_they_should():
    for T in K.ALL_T:
        got = {f for f in K.FAMILIES if K.blocked_set(f, T, T // 3) is not None}
        want = set(K.FAMILIES) - ({"word_boundary"} if T <= 28 else set())
        assert got == want, (T, got)
    assert K.blocked_set("word_boundary", 33, 0) == [28, 29, 30, 31, 32]
    assert K.blocked_set("word_boundary", 300, 0) == list(range(28, 36))


@pytest.mark.parametrize("name", ["tiny4", "dh80"])
def test_negative_control_every_case_moves_the_logits(name):
    """fp64: |knocked - clean| logits > 100 x the GPU test's logit bar, in every end-to-end case."""
    cfg = tvr_amd.get_config("tiny").with_(n_layers=4) if name == "tiny4" else \
        tvr_amd.PythiaConfig(3, 320, 4, 640, 512, n_ctx=256)
    for fp16 in ((False,) if name == "tiny4" else (False, True)):
        sd = tvr_amd.weights.synth_hf_state_dict(cfg, seed=0, std=0.15, fp16=fp16)
        o64 = make_oracle(cfg, sd, tvr_amd.tokenizer.SyntheticTokenizer(cfg.d_vocab), torch.float64)
        for p in K.e2e_prompts(cfg):
            clean = o64(torch.tensor([p]))[0, -1]
            for members, keys in K.e2e_cases(cfg, len(p)):
                ref = K.knocked_logits(o64, p, members, keys)
                moved = (ref - clean).abs().max().item() / ref.abs().max().item()
                print(f"{name} fp16={fp16} T {len(p)} members {len(members)} keys {len(keys)}: moved {moved:.2e}")
                assert moved > 100 * K.LOGIT_TOL, (len(p), members, keys, moved)


def test_facade_reference_leaves_few_prompts_out(tiny4):
    """The margin rule of the façade tests (accuracy compared where the fp64 top-1 margin exceeds
    FACADE_MARGIN x max |logit|) leaves at most 1 prompt in 8 out, per window, on the inputs chosen."""
    import random
    cfg, o64 = tiny4
    prompts, answers, blocked, windows = K.facade_inputs(cfg, o64)
    for heads in (None, [0, 2]):
        ref = K.oracle_effect(o64, prompts, answers, blocked, windows, heads)
        assert ((~ref["margin_ok"]).sum(0) <= len(prompts) // 8).all(), ref["margin_ok"]
        assert ref["top_ko"].any() and not ref["top_ko"].all()  # the accuracies say something
        assert np.abs(ref["p_ko"] - ref["p_clean"][:, None]).max() > 100 * K.PROB_TOL * ref["p_ko"].max()
    host = HostModel(cfg.d_vocab)
    random.seed(K.ROLE_SEED)
    ps, roles, ans = tvr_amd.experiments.knockout_role_prompts(host, list(tvr_amd.tasks.letter_to_caps),
                                                               tvr_amd.tasks.ARROW, ",", K.ROLE_PROMPTS, 2)
    for name in K.ROLE_NAMES:
        idx = tvr_amd.prompts.ROLES.index(name)
        bl = [[j for j, c in enumerate(tr) if c == idx] for tr in roles]
        ref = K.oracle_effect(o64, ps, ans, bl, [(0, 1), (2, 3)], None)
        assert ((~ref["margin_ok"]).sum(0) <= len(ps) // 8).all(), (name, ref["margin_ok"])
