"""The reference's experiment entry points, same names and signatures,
executed as batched sweeps on the HIP engine.

Each function replaces a Python loop of batch-1 TransformerLens forwards
(one per prompt x patch site) with one clean-forward launch sequence and one
patch-sweep launch sequence whose batch enumerates the sites:

  generate_mean_activation                     scratch2.py:81-100   (a1)
  gather_head_activations_to_layers            scratch2.py:103-104  (a2)
  apply_layered_vectors_to_zero_shot           scratch2.py:114-127  (a3, a4)
  apply_layered_vectors_to_zero_shot_by_probability  scratch2.py:135-150 (a5)
  calculate_average_causal_indirect_effect     scratch2.py:171-197  (a6, a7)
  assemble_task_vector                         scratch2.py:232-238  (a10)
  logits_to_next_k_tokens, check_accuracy_of_task_vector,
  check_accuracy_of_added_task_vector          scratch2.py:278-314  (a11)
  test_component_hypothesis                    scratch.py:106-147   (a12)
  substitute_task                              scratch.py:164-213

Beyond the reference's loops (one run_with_hooks call with a scratch2.py:188
hook per head of a set; the function-vector paper's joint mean-ablation):

  joint_head_patch_effect, head_ablation_curve

and Hendel et al.'s residual-stream task vectors (mean of hook_resid_pre at the
function token over ICL prompts, written into a zero-shot prompt's last
position layer by layer):

  extract_task_vectors, apply_task_vectors_to_zero_shot,
  apply_task_vectors_to_zero_shot_by_probability

and the cheap head signal of Todd et al., the last token's attention by token
role (one pass over the trace's Q / K rows, no patched forward):

  head_attention_profile, top_attention_heads

and the two readings of a clean trace through the unembedding: direct logit
attribution (TransformerLens' stack_head_results + logit_attrs; the second cheap
head signal beside the attention profile, on the CIE sweep's own inputs) and the
logit lens / vocabulary decoding of residual rows and of task / function vectors:

  head_logit_attribution, top_attribution_heads, logit_lens_by_layer,
  decode_vectors

and the causal counterpart of the attention profile, attention knockout (Geva et
al. 2023; Wang et al. 2023): block the last token's attention to chosen keys in
a window of layers and re-measure the answer, one sweep for prompts x windows:

  attention_knockout_effect, attention_knockout_by_role

and the product of the two cheap signals, each head's direct logit attribution
split over the roles of the keys it attends to (from which tokens a head
carries the answer's logit; one pass over the trace's Q / K / V rows):

  head_source_attribution, top_source_heads

Drop-in notes
* ``model`` is an ``amd.Model`` instead of a HookedTransformer; it must be
  passed (the reference's defaults bind a module-global model).
* Late-binding closure (App. B1): the reference's layer sweeps add
  ``layered_vectors[-1]`` at every layer.  ``reference_late_binding=True``
  (default) reproduces that; ``False`` adds ``layered_vectors[i]`` at layer i.
* Accuracy compares decoded strings exactly as the reference (B5).
* ``assemble_task_vector`` accepts device tensors (the reference's
  ``.numpy()`` needs CPU tensors, B9).
"""
from __future__ import annotations

import random
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .model import Model, make_sites, range_checked
from .prompts import (Pairs, assemble_end_list_tasks, construct_query, generate_shuffled_prompt,  # noqa: F401
                      ROLES, generate_shuffled_prompts, icl_multi_token, icl_single_token, sample_icl_prompts,
                      sample_icl_prompts_with_roles)

# Sites per patch_sweep launch (bounds the activation workspace: a CIE site
# of a T-token prompt holds T rows).
MAX_SITES_PER_LAUNCH = 16384
# Prompts per clean-forward launch during extraction.
EXTRACT_BATCH = 2048


def _chunks(n: int, size: int):
    """[a, b) ranges of at most ``size`` covering range(n), as equal as
    possible (12 prompts at 11 per launch run as 6 + 6, not 11 + 1: a
    1-prompt launch shares no prefix rows and runs small GEMMs)."""
    if n <= 0:
        return
    k = -(-n // size)
    for i in range(k):
        yield i * n // k, (i + 1) * n // k


# ------------------------------------------------------------------ a1 / a2
@range_checked
def generate_mean_activation(contexts: Pairs, function_token: str, seperator_token: str = ",",
                             model: Model = None, num_contexts: int = 1024, len_contexts: int = 4
                             ) -> torch.Tensor:
    """Mean over ``num_contexts`` ICL prompts of ``blocks.{l}.attn.hook_result``
    at the last position, for every layer and head: [n_layers, n_heads, d_model].
    Captured in z form on the GPU and projected once (mean is linear)."""
    prompts = sample_icl_prompts(model, contexts, function_token, seperator_token, num_contexts,
                                 len_contexts)
    return model.project_heads(sum_last_z(model, prompts)) / num_contexts


@range_checked
def sum_last_z(model: Model, prompts: Sequence[Sequence[int]]) -> torch.Tensor:
    """Σ over prompts of hook_z at the last position, [L, d] (fp32, device)."""
    total = None
    for a, b in _chunks(len(prompts), EXTRACT_BATCH):
        z = model.forward_clean(prompts[a:b], capture=True)["zsum"]
        total = z if total is None else total + z
    return total


def gather_head_activations_to_layers(mean_head_activations: torch.Tensor) -> torch.Tensor:
    return mean_head_activations.sum(1)


# ------------------------------------------------------------- a3 / a4 / a5
def _layer_vectors(layered_vectors: torch.Tensor, model: Model, late_binding: bool):
    v = layered_vectors.to(model.device, torch.float32)
    if late_binding:
        return v[-1:].contiguous(), lambda layer: 0
    if v.shape[0] != model.cfg.n_layers:
        raise ValueError("layered_vectors must have one row per layer")
    return v.contiguous(), lambda layer: layer


def _add_site_outputs(model: Model, seqs: List[List[int]], site_seq, site_layer, site_vec, vectors: torch.Tensor,
                      targets: Optional[List[int]], topk: int, shard=None, clean_outputs: bool = True,
                      kind: int = _lib.SITE_ADD_ATTN_OUT_LASTPOS):
    """Clean forward of ``seqs`` + the last-position vector sites of the global
    site list (site_seq, site_layer, site_vec).  ``kind``: ADD_ATTN_OUT_LASTPOS
    (``hook_attn_out[0, -1] += vectors[vec]`` at ``layer``, scratch2.py:107-109)
    or SET_RESID_PRE_VEC (``hook_resid_pre[0, -1] = vectors[vec]`` at ``layer``,
    then the forward from that layer: Hendel et al.'s task-vector patch).  ``shard``
    (distributed.SiteShard) evaluates only this rank's sites and all-gathers
    the per-site outputs, so every rank returns every site in global order.
    ``clean_outputs=False``: the caller reads no clean outputs, so the clean
    rows skip their final LayerNorm + unembed statistics.
    Returns (clean outputs per prompt, patched outputs per site)."""
    n_sites = len(site_seq)
    sel = np.arange(n_sites) if shard is None else np.asarray(shard.select(n_sites), dtype=np.int64)
    trace = model._sweep_trace(len(seqs), sum(len(s) for s in seqs))
    # the clean rows run inside the first sweep launch when there is one
    clean = model.forward_clean(seqs, targets=targets if clean_outputs else None, topk=topk if clean_outputs else 0,
                                trace=trace, defer=len(sel) > 0)
    dev = model.device
    patched = {}
    if targets is not None:
        patched["prob"] = [torch.empty(0, device=dev)]
    if topk:
        patched["topk"] = [torch.empty(0, topk, dtype=torch.int32, device=dev)]
    if len(sel):
        patched = {k: [] for k in patched}
        sites = make_sites(len(sel))
        sites["kind"] = kind
        sites["seq"] = np.asarray(site_seq)[sel]
        sites["layer"] = np.asarray(site_layer)[sel]
        sites["vec"] = np.asarray(site_vec)[sel]
        if kind == _lib.SITE_SET_RESID_PRE_VEC:  # the patched position: the last one
            sites["pos"] = np.asarray([len(s) for s in seqs], dtype=np.int32)[sites["seq"]] - 1
        if targets is not None:
            sites["target"] = np.asarray(targets)[sites["seq"]]
        for a, b in _chunks(len(sites), MAX_SITES_PER_LAUNCH):
            out = model.patch_sweep(trace, sites[a:b], vectors, topk=topk, want_prob=targets is not None)
            for k in patched:
                patched[k].append(out[k])
    patched = {k: torch.cat(v) for k, v in patched.items()}
    if shard is not None:
        patched = {k: shard.gather(v, n_sites) for k, v in patched.items()}
    return clean, patched


def _injection_sweep(model: Model, seqs: List[List[int]], vectors: torch.Tensor, vec_of_layer,
                     layers: Sequence[int], targets: Optional[List[int]], topk: int, shard=None,
                     clean_outputs: bool = True, kind: int = _lib.SITE_ADD_ATTN_OUT_LASTPOS):
    """One last-position site of ``kind`` (``_add_site_outputs``) per (prompt,
    layer).  Returns (clean outputs, patched outputs [n, len(layers)])."""
    n, layers = len(seqs), list(layers)
    site_layer = np.tile(np.asarray(layers, dtype=np.int32), n)
    site_vec = np.tile(np.asarray([vec_of_layer(l) for l in layers], dtype=np.int32), n)
    clean, patched = _add_site_outputs(model, seqs, np.repeat(np.arange(n, dtype=np.int32), len(layers)), site_layer,
                                       site_vec, vectors, targets, topk, shard, clean_outputs, kind)
    return clean, {k: v.view(n, len(layers), *v.shape[1:]) for k, v in patched.items()}


@range_checked
def _zero_shot_accuracy(layered_vectors, contexts: Pairs, function_token: str, model: Model,
                        reference_late_binding: bool, shard=None,
                        kind: int = _lib.SITE_ADD_ATTN_OUT_LASTPOS) -> List[float]:
    L = model.cfg.n_layers
    vectors, vec_of = _layer_vectors(layered_vectors, model, reference_late_binding)
    f = model.to_single_token(function_token)
    seqs = [[0, model.to_single_token(x), f] for x, _ in contexts]
    _, patched = _injection_sweep(model, seqs, vectors, vec_of, range(L), None, 1, shard, clean_outputs=False,
                                  kind=kind)
    # top-1 decoded == answer (scratch2.py's to_string comparison), decoding
    # each distinct token id once instead of once per (prompt, layer)
    ids, inv = np.unique(patched["topk"][..., 0].cpu().numpy(), return_inverse=True)
    words = [model.to_string(int(t)) for t in ids]
    want = {y: i for i, y in enumerate(dict.fromkeys(y for _, y in contexts))}
    eq = np.array([[w == y for y in want] for w in words], dtype=bool).reshape(len(ids), len(want))
    col = np.asarray([want[y] for _, y in contexts])
    hits = eq[inv.reshape(len(contexts), L), col[:, None]].sum(0)
    return [1.0 * int(h) / len(contexts) for h in hits]


@range_checked
def _zero_shot_dprob(layered_vectors, contexts: Pairs, function_token: str, model: Model,
                     reference_late_binding: bool, shard=None,
                     kind: int = _lib.SITE_ADD_ATTN_OUT_LASTPOS) -> torch.Tensor:
    L = model.cfg.n_layers
    vectors, vec_of = _layer_vectors(layered_vectors, model, reference_late_binding)
    f = model.to_single_token(function_token)
    enc = model.tokenizer.encode
    seqs = [[0] + enc(x) + [f] for x, _ in contexts]
    targets = [enc(y)[0] for _, y in contexts]
    clean, patched = _injection_sweep(model, seqs, vectors, vec_of, range(L), targets, 0, shard, kind=kind)
    return (patched["prob"] - clean["prob"][:, None]).sum(0) / len(contexts)


@range_checked
def apply_layered_vectors_to_zero_shot(layered_vectors: torch.Tensor, contexts: Pairs, function_token: str,
                                       model: Model = None, reference_late_binding: bool = True) -> List[float]:
    """Per-layer top-1 accuracy of zero-shot ``[BOS, x, f]`` prompts with a
    vector added to ``hook_attn_out[0, -1]`` at that layer."""
    return _zero_shot_accuracy(layered_vectors, contexts, function_token, model, reference_late_binding)


@range_checked
def apply_layered_vectors_to_zero_shot_by_probability(layered_vectors: torch.Tensor, contexts: Pairs,
                                                      function_token: str, model: Model = None,
                                                      reference_late_binding: bool = True) -> torch.Tensor:
    """Per-layer mean change of the first answer token's probability
    (patched − clean), [n_layers] on the device."""
    return _zero_shot_dprob(layered_vectors, contexts, function_token, model, reference_late_binding)


# ------------------------------------------------- residual-stream task vectors
def _task_vector_rows(task_vectors: torch.Tensor, cfg) -> torch.Tensor:
    """Rows 0..L-1 of a [L, d] or [L + 1, d] task-vector table (row l is
    written into ``hook_resid_pre[l]``; ``extract_task_vectors``' row L, the
    final residual, has no block to enter).  No engine call."""
    if not isinstance(task_vectors, torch.Tensor) or task_vectors.dim() != 2 or \
            task_vectors.shape[0] not in (cfg.n_layers, cfg.n_layers + 1) or task_vectors.shape[1] != cfg.d_model:
        raise ValueError("task_vectors must be of shape (n_layers, d_model) or (n_layers + 1, d_model)")
    return task_vectors[:cfg.n_layers]


@range_checked
def extract_task_vectors(contexts: Pairs, function_token: str, model: Model = None, num_contexts: int = 1024,
                         len_contexts: int = 4, seperator_token: Optional[str] = None) -> torch.Tensor:
    """Hendel et al.'s task vectors θ(l): the mean over ``num_contexts`` ICL
    prompts (the prompt stream of ``generate_mean_activation``) of
    ``blocks.{l}.hook_resid_pre`` at the last position — the function token of
    the query — for every layer; row L is the final residual.  [L + 1, d] on
    the device.  One clean forward into a trace and one grouped capture
    (``Model.capture_resid``) per ``EXTRACT_BATCH`` prompts."""
    if num_contexts <= 0:
        raise ValueError("num_contexts must be positive")
    if len_contexts < 0 or len_contexts >= len(contexts):
        raise ValueError("len_contexts must be smaller than the number of contexts (demos + one query)")
    prompts = sample_icl_prompts(model, contexts, function_token, seperator_token, num_contexts, len_contexts)
    total = None
    for a, b in _chunks(len(prompts), EXTRACT_BATCH):
        seqs = prompts[a:b]
        trace = model._sweep_trace(len(seqs), sum(len(s) for s in seqs))
        model.forward_clean(seqs, trace=trace)
        total = model.capture_resid(trace, out=total)  # accumulates across the chunks, in chunk order
    return total[0] / num_contexts


@range_checked
def apply_task_vectors_to_zero_shot(task_vectors: torch.Tensor, contexts: Pairs, function_token: str,
                                    model: Model = None) -> List[float]:
    """Per-layer top-1 accuracy of zero-shot ``[BOS, x, f]`` prompts with
    ``task_vectors[l]`` written into ``hook_resid_pre[l][0, -1]`` and the
    forward continued from layer l (Hendel et al.'s patch).  One deferred clean
    forward + one SET_RESID_PRE_VEC site per (prompt, layer)."""
    rows = _task_vector_rows(task_vectors, model.cfg)
    return _zero_shot_accuracy(rows, contexts, function_token, model, False, kind=_lib.SITE_SET_RESID_PRE_VEC)


@range_checked
def apply_task_vectors_to_zero_shot_by_probability(task_vectors: torch.Tensor, contexts: Pairs, function_token: str,
                                                   model: Model = None) -> torch.Tensor:
    """Per-layer mean change of the first answer token's probability (patched
    − clean) under the same patch, prompts ``[BOS] + enc(x) + [f]``.
    [n_layers] on the device."""
    rows = _task_vector_rows(task_vectors, model.cfg)
    return _zero_shot_dprob(rows, contexts, function_token, model, False, kind=_lib.SITE_SET_RESID_PRE_VEC)


# ---------------------------------------------------- attention by token role
@range_checked
def head_attention_profile(contexts: Pairs, function_token: str, seperator_token: Optional[str] = None,
                           model: Model = None, num_contexts: int = 256, len_contexts: int = 4) -> torch.Tensor:
    """Where the last token of an ICL prompt attends, per head: the mean over
    ``num_contexts`` prompts (the prompt stream of ``generate_mean_activation``)
    of ``blocks.{l}.attn.hook_pattern[0, h, -1, :]`` summed over the tokens of
    each role of ``prompts.ROLES``.  [n_layers, n_heads, len(ROLES)] on the
    device; every (l, h) row sums to 1.  The cheap companion of
    ``calculate_average_causal_indirect_effect`` (Todd et al. describe
    function-vector heads by their attention to the demonstrations' labels):
    one clean forward into a trace and one pass over its Q / K rows
    (``Trace.attention_mass``) per ``EXTRACT_BATCH`` prompts, no patched
    forward."""
    if num_contexts <= 0:
        raise ValueError("num_contexts must be positive")
    if len_contexts < 0 or len_contexts >= len(contexts):
        raise ValueError("len_contexts must be smaller than the number of contexts (demos + one query)")
    prompts, roles = sample_icl_prompts_with_roles(model, contexts, function_token, seperator_token, num_contexts,
                                                   len_contexts)
    total = None
    for a, b in _chunks(len(prompts), EXTRACT_BATCH):
        seqs = prompts[a:b]
        trace = model._sweep_trace(len(seqs), sum(len(s) for s in seqs))
        model.forward_clean(seqs, trace=trace)
        mass = trace.attention_mass(roles[a:b], len(ROLES)).sum(0)  # prompts in order: reproducible
        total = mass if total is None else total + mass
    return total / num_contexts


def top_attention_heads(profile: torch.Tensor, role, num_heads: int) -> List[Tuple[int, int]]:
    """The ``num_heads`` (layer, head) pairs of a ``head_attention_profile``
    that put the most attention on ``role`` (a name of ``prompts.ROLES`` or its
    index), highest first (torch.topk's order and tie rule, as
    ``top_cie_heads``)."""
    if not isinstance(profile, torch.Tensor) or profile.dim() != 3 or profile.shape[2] != len(ROLES):
        raise ValueError("profile must be of shape (n_layers, n_heads, len(ROLES))")
    if isinstance(role, str):
        if role not in ROLES:
            raise ValueError(f"role must be one of {ROLES}")
        role = ROLES.index(role)
    if not 0 <= int(role) < len(ROLES):
        raise ValueError(f"role must be one of {ROLES} or its index")
    H = profile.shape[1]
    if not 0 < num_heads <= profile.shape[0] * H:
        raise ValueError("num_heads must be in [1, n_layers * n_heads]")
    _, idx = torch.topk(profile[:, :, int(role)].flatten(), num_heads)
    return [(int(i) // H, int(i) % H) for i in idx.tolist()]


# ------------------------------------------------ direct logit attribution / logit lens
class HeadLogitAttribution(NamedTuple):
    """Means over prompts of the direct logit attribution of the answer token at
    the last position (``head_logit_attribution``)."""
    heads: torch.Tensor   # [n_layers, n_heads]: each head's hook_result
    rest: torch.Tensor    # [n_layers]: the layer's MLP and its biases (b_O + b_out are merged in the engine)
    embed: torch.Tensor   # []: the embedding
    total: torch.Tensor   # []: the final residual = logit[answer] (− logit[contrast]) minus b_U's share


def _check_prompts_answers(scrambled_prompts, prompt_answers, contrast_answers=None):
    if len(scrambled_prompts) == 0:
        raise ValueError("no prompts")
    if len(scrambled_prompts) != len(prompt_answers):
        raise ValueError("Prompt answers must be of the same length as scrambled prompts")
    if contrast_answers is not None and len(contrast_answers) != len(scrambled_prompts):
        raise ValueError("Contrast answers must be of the same length as scrambled prompts")


@range_checked
def head_logit_attribution(scrambled_prompts, prompt_answers, model: Model = None,
                           contrast_answers=None) -> HeadLogitAttribution:
    """Direct logit attribution of each prompt's answer token (its first token,
    as the CIE sweep scores it) at the last position, averaged over prompts:
    how much every head, every layer's MLP and biases, and the embedding push
    the answer's logit (or, with ``contrast_answers``, the logit difference),
    through the final LayerNorm's scale.  Prompts and answers in the forms
    ``calculate_average_causal_indirect_effect`` takes, so both rank the same
    heads on the same prompts; this one needs one clean forward into a trace
    and one pass over it (``Trace.logit_attribution``) per ``EXTRACT_BATCH``
    prompts, no patched forward.  ``rest[l] = resid[l + 1] − resid[l] −
    Σ_h heads[l, h]``."""
    _check_prompts_answers(scrambled_prompts, prompt_answers, contrast_answers)
    prompts, answers = normalize_cie_inputs(model, scrambled_prompts, prompt_answers)
    contrast = normalize_cie_inputs(model, [], contrast_answers)[1] if contrast_answers is not None else None
    heads = resid = None
    for a, b in _chunks(len(prompts), EXTRACT_BATCH):
        seqs = prompts[a:b]
        trace = model._sweep_trace(len(seqs), sum(len(s) for s in seqs))
        model.forward_clean(seqs, trace=trace)
        h, r = trace.logit_attribution(answers[a:b], contrast=contrast[a:b] if contrast is not None else None)
        h, r = h.sum(0), r.sum(0)  # prompts in order: reproducible
        heads, resid = (h, r) if heads is None else (heads + h, resid + r)
    heads, resid = heads / len(prompts), resid / len(prompts)
    rest = resid[1:] - resid[:-1] - heads.sum(1)
    return HeadLogitAttribution(heads, rest, resid[0], resid[-1])


def top_attribution_heads(heads: torch.Tensor, num_heads: int) -> List[Tuple[int, int]]:
    """The ``num_heads`` (layer, head) pairs with the largest attribution of a
    ``head_logit_attribution(...).heads``, highest first (torch.topk's order and
    tie rule, as ``top_cie_heads``)."""
    if not isinstance(heads, torch.Tensor) or heads.dim() != 2:
        raise ValueError("heads must be of shape (n_layers, n_heads)")
    H = heads.shape[1]
    if not 0 < num_heads <= heads.shape[0] * H:
        raise ValueError("num_heads must be in [1, n_layers * n_heads]")
    _, idx = torch.topk(heads.flatten(), num_heads)
    return [(int(i) // H, int(i) % H) for i in idx.tolist()]


@range_checked
def logit_lens_by_layer(scrambled_prompts, prompt_answers, model: Model = None, topk: int = 1):
    """The logit lens over prompts: for every layer ``l`` in ``[0, n_layers]`` the
    share of prompts whose answer token (first token) is among the top ``topk``
    tokens decoded from ``hook_resid_pre[l]`` at the last position (``l =
    n_layers``: the model's own prediction), and the mean probability of the
    answer there.  Returns ``(accuracy [n_layers + 1], probability [n_layers + 1])``."""
    _check_prompts_answers(scrambled_prompts, prompt_answers)
    if not 1 <= int(topk) <= _lib.STATS_MAX_K:
        raise ValueError(f"topk must be in [1, {_lib.STATS_MAX_K}]")
    prompts, answers = normalize_cie_inputs(model, scrambled_prompts, prompt_answers)
    hits = prob = None
    for a, b in _chunks(len(prompts), EXTRACT_BATCH):
        seqs = prompts[a:b]
        trace = model._sweep_trace(len(seqs), sum(len(s) for s in seqs))
        model.forward_clean(seqs, trace=trace)
        p, top = trace.logit_lens(answers[a:b], topk=int(topk))
        tg = torch.as_tensor(answers[a:b], dtype=torch.int32, device=model.device)
        h = (top == tg[:, None, None]).any(-1).sum(0)
        p = p.sum(0)
        hits, prob = (h, p) if hits is None else (hits + h, prob + p)
    return hits.to(torch.float32) / len(prompts), prob / len(prompts)


@range_checked
def decode_vectors(vectors: torch.Tensor, k: int, model: Model = None) -> List[List[str]]:
    """The ``k`` most likely next tokens each vector ``[n, d_model]`` (or one
    ``[d_model]``) encodes, decoded through the final LayerNorm and the
    unembedding, most likely first: the tables of decoded task vectors (Hendel
    et al.) and function vectors (Todd et al.)."""
    if not isinstance(vectors, torch.Tensor) or vectors.dim() not in (1, 2) or \
            vectors.shape[-1] != model.cfg.d_model or vectors.numel() == 0:
        raise ValueError("vectors must be of shape (n, d_model) or (d_model,)")
    if not 1 <= int(k) <= _lib.STATS_MAX_K:
        raise ValueError(f"k must be in [1, {_lib.STATS_MAX_K}]")
    rows = vectors.to(model.device, torch.float32).reshape(-1, model.cfg.d_model)
    _, top = model.decode_rows(rows, topk=int(k))
    return [[model.to_string(t) for t in row] for row in top.tolist()]


# ------------------------------------------------------------------- a6 / a7
def normalize_cie_inputs(model: Model, scrambled_prompts, prompt_answers):
    """The reference's prompt / answer forms → token-id prompts (BOS
    prepended to strings by ``to_tokens``, scratch2.py:182) and first answer
    token ids (``[answer][0]``, scratch2.py:184,192: B3)."""
    prompts = [model.to_tokens(p)[0].tolist() if isinstance(p, str) else [int(x) for x in p]
               for p in scrambled_prompts]
    answers = [int(a[0]) if isinstance(a, (list, tuple)) else int(a) for a in prompt_answers]
    return prompts, answers


@range_checked
def causal_indirect_effect_sums(mean_head_activations: torch.Tensor, prompts: Sequence[Sequence[int]],
                                answers: Sequence[int], model: Model,
                                layers: Optional[Sequence[int]] = None,
                                heads: Optional[Sequence[int]] = None,
                                sites: Optional[Sequence[Tuple[int, int]]] = None) -> torch.Tensor:
    """Σ over prompts of p_patched(answer) − p_clean(answer) for every
    (layer, head) site, [n_layers, n_heads] (zeros outside ``layers``/``heads``,
    or outside the explicit (layer, head) list ``sites``).
    ``prompts`` are token ids (BOS included); one clean forward + one
    staircase sweep per launch-sized group of prompts."""
    cfg = model.cfg
    L, H = cfg.n_layers, cfg.n_heads
    if sites is not None:
        if layers is not None or heads is not None:
            raise ValueError("give either sites or layers / heads")
        sl = np.asarray(sites, dtype=np.int32).reshape(-1, 2)
        if sl.size and (sl[:, 0].min() < 0 or sl[:, 0].max() >= L or sl[:, 1].min() < 0 or sl[:, 1].max() >= H):
            raise ValueError("site (layer, head) out of range")
        grid_l, grid_h = sl[:, 0].copy(), sl[:, 1].copy()
    else:
        layers = list(range(L)) if layers is None else list(layers)
        heads = list(range(H)) if heads is None else list(heads)
        grid_l = np.repeat(np.asarray(layers, dtype=np.int32), len(heads))
        grid_h = np.tile(np.asarray(heads, dtype=np.int32), len(layers))
    per_prompt = grid_l.size
    vectors = mean_head_activations.to(model.device, torch.float32).reshape(L * H, cfg.d_model).contiguous()
    out = torch.zeros(L, H, device=model.device)
    group = max(1, MAX_SITES_PER_LAUNCH // max(per_prompt, 1))
    for a, b in _chunks(len(prompts), group):
        seqs = [list(map(int, p)) for p in prompts[a:b]]
        tg = [int(t) for t in answers[a:b]]
        n = len(seqs)
        trace = model._sweep_trace(n, sum(len(s) for s in seqs))
        p0 = model.forward_clean(seqs, targets=tg, trace=trace, defer=per_prompt > 0)["prob"]
        sites = make_sites(n * per_prompt)
        sites["seq"] = np.repeat(np.arange(n, dtype=np.int32), per_prompt)
        sites["kind"] = _lib.SITE_REPLACE_HEAD_ALLPOS
        sites["layer"] = np.tile(grid_l, n)
        sites["head"] = np.tile(grid_h, n)
        sites["vec"] = sites["layer"] * H + sites["head"]
        sites["target"] = np.repeat(np.asarray(tg, dtype=np.int32), per_prompt)
        p = model.patch_sweep(trace, sites, vectors)["prob"].view(n, per_prompt)
        delta = (p - p0[:, None]).sum(0)
        out.index_put_((torch.as_tensor(grid_l, device=model.device).long(),
                        torch.as_tensor(grid_h, device=model.device).long()), delta, accumulate=True)
    return out


@range_checked
def calculate_average_causal_indirect_effect(mean_head_activations: torch.Tensor, scrambled_prompts,
                                             prompt_answers, model: Model = None) -> torch.Tensor:
    """CIE[l, h] = mean over prompts of softmax(patched)[answer[0]] −
    softmax(clean)[answer[0]], where the patch writes ``mean[l, h]`` into
    ``hook_result[0, :, h]`` at every position.  [n_layers, n_heads]."""
    cfg = model.cfg
    if tuple(mean_head_activations.shape) != (cfg.n_layers, cfg.n_heads, cfg.d_model):
        raise ValueError("Mean head activations must be of shape (n_layers, n_heads, d_model)")
    if len(scrambled_prompts) != len(prompt_answers):
        raise ValueError("Prompt answers must be of the same length as scrambled prompts")
    prompts, answers = normalize_cie_inputs(model, scrambled_prompts, prompt_answers)
    return causal_indirect_effect_sums(mean_head_activations, prompts, answers, model) / len(prompts)


# ---------------------------------------------------------------- a10 / a11
def _top_cie_index(causal_indirect_effects: torch.Tensor, layer: int, num_heads: int):
    """Flat indices (l * H + h, torch.topk order and tie rule) of the
    ``num_heads`` highest-CIE heads in layers ≤ ``layer``, and H: the head
    selection ``assemble_task_vector`` and ``head_ablation_curve`` share."""
    sub = causal_indirect_effects[: layer + 1, :]
    _, idx = torch.topk(sub.flatten(), num_heads)
    return idx, sub.shape[1]


def top_cie_heads(causal_indirect_effects: torch.Tensor, layer: int, num_heads: int) -> List[Tuple[int, int]]:
    """The (layer, head) pairs whose means ``assemble_task_vector(.., layer,
    num_heads)`` sums, in its order."""
    idx, H = _top_cie_index(causal_indirect_effects, layer, num_heads)
    return [(int(i) // H, int(i) % H) for i in idx.tolist()]


def assemble_task_vector(mean_head_activations: torch.Tensor, causal_indirect_effects: torch.Tensor,
                         layer: int, num_heads: int) -> torch.Tensor:
    """Sum of the mean outputs of the ``num_heads`` highest-CIE heads in
    layers ≤ ``layer`` (torch.topk order and tie rule, as the reference)."""
    idx, H = _top_cie_index(causal_indirect_effects, layer, num_heads)
    rows = mean_head_activations[(idx // H).to(mean_head_activations.device),
                                 (idx % H).to(mean_head_activations.device)]
    vec = torch.zeros(mean_head_activations.shape[-1], dtype=mean_head_activations.dtype,
                      device=mean_head_activations.device)
    for r in rows:  # sequential adds, the reference's summation order
        vec += r
    return vec


def logits_to_next_k_tokens(k: int, logits: torch.Tensor, model: Model = None) -> List[str]:
    return [model.to_string(e) for e in torch.topk(logits[0, -1, :], k).indices.tolist()]


def _fv_topk(task_vector, layer: int, contexts: Pairs, topk: int, model: Model, with_baseline: bool):
    seqs = [model.to_tokens(x + ":")[0].tolist() for x, _ in contexts]
    firsts = [model.to_string(model.tokenizer.encode(y)[0]) for _, y in contexts]
    vec = task_vector.to(model.device, torch.float32).reshape(1, -1).contiguous()
    clean, patched = _injection_sweep(model, seqs, vec, lambda l: 0, [layer], None, topk=topk,
                                      clean_outputs=with_baseline)
    def hits(top):
        return sum(first in [model.to_string(t) for t in row] for first, row in zip(firsts, top.tolist()))
    fv = hits(patched["topk"][:, 0].cpu())
    base = hits(clean["topk"].cpu()) if with_baseline else None
    return base, fv


@range_checked
def check_accuracy_of_task_vector(task_vector: torch.Tensor, layer: int, contexts: Pairs, topk: int = 5,
                                  model: Model = None) -> Tuple[float, float]:
    """(zero-shot top-k accuracy, top-k accuracy with the FV added to
    ``hook_attn_out[0, -1]`` at ``layer``) for prompts ``x + ":"``."""
    base, fv = _fv_topk(task_vector, layer, contexts, topk, model, True)
    return (1.0 * base / len(contexts), 1.0 * fv / len(contexts))


@range_checked
def check_accuracy_of_added_task_vector(task_vector: torch.Tensor, layer: int, contexts: Pairs, topk: int = 5,
                                        model: Model = None) -> float:
    _, fv = _fv_topk(task_vector, layer, contexts, topk, model, False)
    return 1.0 * fv / len(contexts)


# ---------------------------------------------------------------------- a12
@range_checked
def test_component_hypothesis(contexts: Pairs, function_token: str, model: Model = None,
                              num_contexts: int = 256, len_contexts: int = 4, batch_contexts: int = 512):
    """Layer sweep of residual patching: the ICL run's ``hook_resid_pre[L][-2]``
    written into a dummy-query run, continued from layer L.  Returns
    (total, baseline hits, regular hits, [hits per layer])."""
    L = model.cfg.n_layers
    pool = list(contexts)
    draws = []
    for _ in range(num_contexts):
        random.shuffle(pool)
        demos, query = pool[:len_contexts], pool[len_contexts]
        draws.append((demos, query, pool[len_contexts + 1][0]))
    base_hits = normal_hits = 0
    per_layer = [0] * L
    for a, b in _chunks(len(draws), batch_contexts):
        seqs, answers = [], []
        for demos, query, dummy in draws[a:b]:
            seqs.append(model.to_tokens(construct_query(query, function_token)[0])[0].tolist())
            seqs.append(icl_single_token(model, demos, query[0], function_token, None))
            seqs.append(icl_single_token(model, demos, dummy, function_token, None))
            answers.append(query[1])
        n = len(answers)
        trace = model._sweep_trace(3 * n, sum(len(s) for s in seqs))
        top = model.forward_clean(seqs, topk=1, trace=trace)["topk"][:, 0].cpu().view(n, 3).tolist()
        sites = make_sites(n * L)
        T = np.asarray([len(seqs[3 * i + 2]) for i in range(n)], dtype=np.int32)
        sites["kind"] = _lib.SITE_SET_RESID_PRE_POS
        sites["seq"] = np.repeat(3 * np.arange(n) + 2, L)
        sites["src_seq"] = np.repeat(3 * np.arange(n) + 1, L)
        sites["pos"] = np.repeat(T - 2, L)
        sites["src_pos"] = np.repeat(T - 2, L)
        sites["layer"] = np.tile(np.arange(L), n)
        pt = model.patch_sweep(trace, sites, None, topk=1, want_prob=False)["topk"][:, 0].cpu().view(n, L).tolist()
        for i, ans in enumerate(answers):
            base_hits += model.to_string(top[i][0]) == ans
            normal_hits += model.to_string(top[i][1]) == ans
            for l in range(L):
                per_layer[l] += model.to_string(pt[i][l]) == ans
    return (num_contexts, base_hits, normal_hits, per_layer)


@range_checked
def substitute_task(taskA: Pairs, taskB: Pairs, layer: int, function_token: str = "→", model: Model = None,
                    num_contexts: int = 256, len_contexts: int = 4):
    """Swap ``hook_resid_pre[layer][-1]`` between a task-A and a task-B run of
    the same query.  Returns (n, A hits, B hits, A←B hits on B's answer,
    B←A hits on A's answer).  Sorts both task lists in place (App. B6)."""
    if len(taskA) != len(taskB):
        raise ValueError("The two tasks must have the same length")
    taskA.sort(key=lambda p: p[0])
    taskB.sort(key=lambda p: p[0])
    if any(a[0] != b[0] for a, b in zip(taskA, taskB)):
        raise ValueError("The two tasks must have the same domains")
    mixed = [(a[0], a[1], b[1]) for a, b in zip(taskA, taskB)]
    seqs, ans = [], []
    for _ in range(num_contexts):
        random.shuffle(mixed)
        ctx_a = [(m[0], m[1]) for m in mixed[:len_contexts]]
        ctx_b = [(m[0], m[2]) for m in mixed[:len_contexts]]
        q = mixed[len_contexts][0][0]  # first character of the query item, as scratch.py:189
        seqs.append(icl_single_token(model, ctx_a, q, function_token, None))
        seqs.append(icl_single_token(model, ctx_b, q, function_token, None))
        ans.append((mixed[len_contexts][1], mixed[len_contexts][2]))
    n = num_contexts
    trace = model._sweep_trace(2 * n, sum(len(s) for s in seqs))
    top = model.forward_clean(seqs, topk=1, trace=trace)["topk"][:, 0].cpu().view(n, 2).tolist()
    sites = make_sites(2 * n)
    T = np.asarray([len(s) for s in seqs], dtype=np.int32)
    sites["kind"] = _lib.SITE_SET_RESID_PRE_POS
    sites["layer"] = layer
    sites["seq"] = np.arange(2 * n)
    sites["src_seq"] = np.arange(2 * n) ^ 1  # A takes B's row, B takes A's
    sites["pos"] = T - 1
    sites["src_pos"] = T[np.arange(2 * n) ^ 1] - 1
    pt = model.patch_sweep(trace, sites, None, topk=1, want_prob=False)["topk"][:, 0].cpu().view(n, 2).tolist()
    a_hits = sum(model.to_string(top[i][0]) == ans[i][0] for i in range(n))
    b_hits = sum(model.to_string(top[i][1]) == ans[i][1] for i in range(n))
    a_to_b = sum(model.to_string(pt[i][0]) == ans[i][1] for i in range(n))
    b_to_a = sum(model.to_string(pt[i][1]) == ans[i][0] for i in range(n))
    return (num_contexts, a_hits, b_hits, a_to_b, b_to_a)


# ------------------------------------------------------- batched FV evaluation
def _fv_sites_topk(model: Model, contexts: Pairs, vectors: torch.Tensor, layer_vec: Sequence[Tuple[int, int]],
                   topk: int, shard=None):
    """Top-k hits of every (prompt, (layer, vector)) pair in ONE sweep:
    prompts ``x + ":"``, vector added to hook_attn_out[0, -1] at the layer
    (scratch2.py:306-314 semantics).  Returns hits [len(layer_vec)]."""
    seqs = [model.to_tokens(x + ":")[0].tolist() for x, _ in contexts]
    firsts = [model.to_string(model.tokenizer.encode(y)[0]) for _, y in contexts]
    n, m = len(seqs), len(layer_vec)
    lv = np.asarray(layer_vec, dtype=np.int32).reshape(m, 2)
    vecs = vectors.to(model.device, torch.float32).reshape(-1, model.cfg.d_model).contiguous()
    _, patched = _add_site_outputs(model, seqs, np.repeat(np.arange(n, dtype=np.int32), m), np.tile(lv[:, 0], n),
                                   np.tile(lv[:, 1], n), vecs, None, topk, shard, clean_outputs=False)
    top = patched["topk"].view(n, m, topk).cpu().tolist()
    hits = np.zeros(m, dtype=np.int64)
    for i, first in enumerate(firsts):
        for j in range(m):
            hits[j] += first in [model.to_string(t) for t in top[i][j]]
    return hits


@range_checked
def check_accuracy_of_added_task_vector_by_layer(task_vector: torch.Tensor, contexts: Pairs, topk: int = 5,
                                                 model: Model = None, shard=None) -> List[float]:
    """``check_accuracy_of_added_task_vector`` at every layer (one sweep;
    ``shard``: distributed.SiteShard, sites round-robin over ranks)."""
    L = model.cfg.n_layers
    hits = _fv_sites_topk(model, contexts, task_vector.reshape(1, -1), [(l, 0) for l in range(L)], topk, shard)
    return [float(h) / len(contexts) for h in hits]


@range_checked
def function_vector_head_count_grid(mean_head_activations: torch.Tensor, causal_indirect_effects: torch.Tensor,
                                    contexts: Pairs, model: Model = None, heads_per_batch: int = 2,
                                    number_of_batches: int = 64, topk: int = 5, shard=None) -> torch.Tensor:
    """The FV head-count grid of scratch2.py:411-425 as ONE batched sweep:
    accuracy[i, j] of the function vector made of the top (j+1)*heads_per_batch
    heads of layers <= i, added at layer i.  Where the reference skips the
    assembly ((j+1)*k >= (i+1)*n_heads, :416) its ``task_vectors[i, j]`` stays
    the zero vector it was created as (:413) and the accuracy loop (:420-424)
    still evaluates it: those cells are the zero vector added at layer i, i.e.
    layer i's zero-shot top-k accuracy.  [n_layers, number_of_batches]."""
    L, H = model.cfg.n_layers, model.cfg.n_heads
    d = mean_head_activations.shape[-1]
    vecs = [torch.zeros(d, dtype=torch.float32, device=model.device)]  # vector 0: the skipped cells
    cells = []  # (i, j, index of the evaluated (layer, vector) pair)
    pairs = []
    for i in range(L):
        zero_pair = None  # layer i's skipped cells share ONE (layer i, zero vector) evaluation
        for j in range(number_of_batches):
            k = (j + 1) * heads_per_batch
            if k < (i + 1) * H:
                vecs.append(assemble_task_vector(mean_head_activations, causal_indirect_effects, i, k)
                            .to(model.device, torch.float32))
                pairs.append((i, len(vecs) - 1))
                cells.append((i, j, len(pairs) - 1))
            else:
                if zero_pair is None:
                    pairs.append((i, 0))
                    zero_pair = len(pairs) - 1
                cells.append((i, j, zero_pair))
    hits = _fv_sites_topk(model, contexts, torch.stack(vecs), pairs, topk, shard)
    acc = torch.zeros(L, number_of_batches)
    for i, j, q in cells:
        acc[i, j] = float(hits[q]) / len(contexts)
    return acc


# ------------------------------------------------------ joint head-set patching
# Rows per patch_sweep_sets launch: an all-positions set site of a T-token
# prompt holds T rows whatever its size (MAX_SITES_PER_LAUNCH CIE sites of 16
# tokens: the workspace the CIE sweep already reaches).
MAX_ROWS_PER_LAUNCH = 16 * MAX_SITES_PER_LAUNCH
POSITION_KINDS = {"all": _lib.SITE_REPLACE_HEADSET_ALLPOS, "last": _lib.SITE_REPLACE_HEADSET_LASTPOS}


def _check_head_sets(cfg, mean_head_activations, head_sets, n_prompts: int, n_answers: int, positions: str):
    """Argument checks of the joint head-set functions (no engine call).
    Returns the sets as lists of (layer, head) int pairs."""
    if tuple(mean_head_activations.shape) != (cfg.n_layers, cfg.n_heads, cfg.d_model):
        raise ValueError("Mean head activations must be of shape (n_layers, n_heads, d_model)")
    if n_prompts != n_answers:
        raise ValueError("Prompt answers must be of the same length as scrambled prompts")
    if positions not in POSITION_KINDS:
        raise ValueError(f"positions must be one of {sorted(POSITION_KINDS)}, got {positions!r}")
    sets = []
    for s in head_sets:
        pairs = [(int(l), int(h)) for l, h in s]
        if any(not (0 <= l < cfg.n_layers and 0 <= h < cfg.n_heads) for l, h in pairs):
            raise ValueError("head set (layer, head) out of range")
        if len(set(pairs)) != len(pairs):
            raise ValueError("the same (layer, head) twice in one head set")
        sets.append(pairs)
    return sets


@range_checked
def joint_head_patch_effect(mean_head_activations: torch.Tensor, head_sets, scrambled_prompts, prompt_answers,
                            model: Model = None, positions: str = "all", topk: int = 1) -> dict:
    """Patch every head of a SET at once: for each set of ``head_sets`` (lists
    of (layer, head)) and each prompt, one forward with
    ``hook_result[0, :, h] = mean[l, h]`` (``positions="all"``, the reference's
    hook, scratch2.py:188) or ``hook_result[0, -1, h] = mean[l, h]``
    (``"last"``, the function-vector paper's) for every member (l, h), scoring
    the first answer token (B3).  Prompts and answers as
    ``calculate_average_causal_indirect_effect``.  Returns ``dprob`` [n_sets]
    (mean over prompts of p_patched − p_clean, device), ``accuracy`` [n_sets]
    (share of prompts whose answer token is in the patched top-``topk``),
    ``clean_prob`` and ``clean_accuracy`` (floats).  Means of a corrupted task
    give the joint mean-ablation of Todd et al. §3, means of the clean task
    joint sufficiency.  One clean forward + one sweep per launch-sized group."""
    cfg = model.cfg
    sets = _check_head_sets(cfg, mean_head_activations, head_sets, len(scrambled_prompts), len(prompt_answers),
                            positions)
    if topk < 1:
        raise ValueError("topk must be at least 1")
    prompts, answers = normalize_cie_inputs(model, scrambled_prompts, prompt_answers)
    L, H, dev = cfg.n_layers, cfg.n_heads, model.device
    n_sets, n_prompts = len(sets), len(prompts)
    if n_prompts == 0:
        raise ValueError("no prompts")
    vectors = mean_head_activations.to(dev, torch.float32).reshape(L * H, cfg.d_model).contiguous()
    # one prompt's sets as (offsets, patches) relative to the prompt's first site
    sizes = np.asarray([len(s) for s in sets], dtype=np.int64)
    flat = np.asarray([(l, h, l * H + h) for s in sets for l, h in s], dtype=np.int32).reshape(-1, 3)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    maxT = max(len(p) for p in prompts)
    rows_per_site = maxT if positions == "all" else 1
    # chunk by rows, not only by sites: the sets of one launch, then the prompts of one launch
    set_chunk = max(1, min(n_sets, MAX_SITES_PER_LAUNCH, MAX_ROWS_PER_LAUNCH // rows_per_site))
    group = max(1, min(MAX_SITES_PER_LAUNCH, MAX_ROWS_PER_LAUNCH // rows_per_site) // max(min(n_sets, set_chunk), 1))
    dsum = torch.zeros(n_sets, device=dev)
    hits = torch.zeros(n_sets, device=dev)
    clean_p = clean_hits = 0.0
    for a, b in _chunks(n_prompts, group):
        seqs = [list(map(int, p)) for p in prompts[a:b]]
        tg = np.asarray(answers[a:b], dtype=np.int32)
        n = len(seqs)
        trace = model._sweep_trace(n, sum(len(s) for s in seqs))
        clean = model.forward_clean(seqs, targets=tg.tolist(), topk=topk, trace=trace, defer=n_sets > 0)
        tgd = torch.as_tensor(tg, device=dev)
        for sa, sb in _chunks(n_sets, set_chunk):
            m = sb - sa
            sites = make_sites(n * m)
            sites["seq"] = np.repeat(np.arange(n, dtype=np.int32), m)
            sites["kind"] = POSITION_KINDS[positions]
            sites["target"] = np.repeat(tg, m)
            lens = np.tile(sizes[sa:sb], n)
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            pat = np.tile(flat[starts[sa]:starts[sb]], (n, 1))
            out = model.patch_sweep_sets(trace, sites, off, pat, vectors, topk=topk)
            p = out["prob"].view(n, m)
            dsum[sa:sb] += (p - clean["prob"][:, None]).sum(0)
            hits[sa:sb] += (out["topk"].view(n, m, topk) == tgd[:, None, None]).any(-1).sum(0)
        # (the deferred clean outputs are written by the group's first sweep; without sets the forward ran at once)
        clean_p += float(clean["prob"].sum())
        clean_hits += float((clean["topk"] == tgd[:, None]).any(-1).sum())
    return {"dprob": dsum / n_prompts, "accuracy": hits / n_prompts, "clean_prob": clean_p / n_prompts,
            "clean_accuracy": clean_hits / n_prompts}


@range_checked
def head_ablation_curve(mean_head_activations: torch.Tensor, causal_indirect_effects: torch.Tensor,
                        scrambled_prompts, prompt_answers, model: Model = None,
                        counts: Sequence[int] = (1, 2, 5, 10, 20), layer: Optional[int] = None, n_random: int = 0,
                        seed: int = 0, positions: str = "all", topk: int = 1) -> dict:
    """For each k of ``counts``: jointly patch the k highest-CIE heads of
    layers ≤ ``layer`` (default: every layer; ``assemble_task_vector``'s
    selection and tie order) with their rows of ``mean_head_activations``, and
    ``n_random`` control sets of k heads drawn from the same layers with
    ``random.Random(seed)`` (for each k in turn, ``n_random`` calls of
    ``sample(all (l, h) of those layers in row-major order, k)``).  Means of a
    corrupted or unrelated task give the ablation curve of Todd et al. §3,
    means of the clean task joint sufficiency.  Returns ``counts``, ``heads``
    (the top-k list per k), ``random_heads`` (per k, ``n_random`` lists),
    ``top`` (``dprob`` / ``accuracy`` [len(counts)]), ``random`` (the same,
    [len(counts), n_random]), ``clean_prob`` and ``clean_accuracy``: all from
    ONE ``joint_head_patch_effect`` call."""
    cfg = model.cfg
    layer = cfg.n_layers - 1 if layer is None else int(layer)
    if not 0 <= layer < cfg.n_layers:
        raise ValueError("layer out of range")
    if tuple(causal_indirect_effects.shape) != (cfg.n_layers, cfg.n_heads):
        raise ValueError("Causal indirect effects must be of shape (n_layers, n_heads)")
    counts = [int(k) for k in counts]
    pool = [(l, h) for l in range(layer + 1) for h in range(cfg.n_heads)]
    if any(k < 1 or k > len(pool) for k in counts):
        raise ValueError("every count must be between 1 and the number of heads in layers <= layer")
    if n_random < 0:
        raise ValueError("n_random must not be negative")
    rng = random.Random(seed)
    heads = [top_cie_heads(causal_indirect_effects, layer, k) for k in counts]
    random_heads = [[rng.sample(pool, k) for _ in range(n_random)] for k in counts]
    sets = heads + [s for per_k in random_heads for s in per_k]
    r = joint_head_patch_effect(mean_head_activations, sets, scrambled_prompts, prompt_answers, model=model,
                                positions=positions, topk=topk)
    nk = len(counts)
    return {"counts": counts, "heads": heads, "random_heads": random_heads,
            "top": {"dprob": r["dprob"][:nk], "accuracy": r["accuracy"][:nk]},
            "random": {"dprob": r["dprob"][nk:].view(nk, n_random), "accuracy": r["accuracy"][nk:].view(nk, n_random)},
            "clean_prob": r["clean_prob"], "clean_accuracy": r["clean_accuracy"]}


# ------------------------------------------------------------ attention knockout
def _check_knockout(cfg, prompts, n_answers: int, blocked, windows, heads, topk: int):
    """Argument checks of ``attention_knockout_effect`` (no engine call).
    Returns (sorted blocked positions per prompt, windows, heads)."""
    if len(prompts) != n_answers:
        raise ValueError("Prompt answers must be of the same length as scrambled prompts")
    if len(blocked) != len(prompts):
        raise ValueError("blocked must hold one list of key positions per prompt")
    if len(prompts) == 0:
        raise ValueError("no prompts")
    if topk < 1:
        raise ValueError("topk must be at least 1")
    wins = [(int(a), int(b)) for a, b in windows]
    if any(not (0 <= a <= b < cfg.n_layers) for a, b in wins):
        raise ValueError("every window must be (first_layer, last_layer) with 0 <= first <= last < n_layers")
    hs = list(range(cfg.n_heads)) if heads is None else [int(h) for h in heads]
    if any(not 0 <= h < cfg.n_heads for h in hs) or len(set(hs)) != len(hs):
        raise ValueError("heads must be distinct head indices in [0, n_heads)")
    keys = []
    for p, b in zip(prompts, blocked):
        ks = sorted({int(j) for j in b})
        if ks and (ks[0] < 0 or ks[-1] >= len(p)):
            raise ValueError("blocked key position outside the prompt")
        if len(ks) >= len(p):
            raise ValueError("blocked removes every key of a prompt: one key of the last token must remain")
        keys.append(ks)
    return keys, wins, hs


@range_checked
def attention_knockout_effect(scrambled_prompts, prompt_answers, blocked, windows, model: Model = None,
                              heads: Optional[Sequence[int]] = None, topk: int = 1) -> dict:
    """Attention knockout (Geva et al. 2023; Wang et al. 2023): for each prompt
    ``i`` and each window ``(first_layer, last_layer)`` (inclusive), one forward
    in which the LAST token cannot attend to the key positions ``blocked[i]`` —
    ``hook_attn_scores[0, h, -1, j] = -inf`` — in the heads ``heads`` (default:
    all) of every layer of the window, scoring the first answer token (B3).
    Prompts and answers as ``calculate_average_causal_indirect_effect``.
    Returns ``dprob`` [n_windows] (mean over prompts of p_knocked − p_clean,
    device), ``rel_dprob`` (mean of (p_knocked − p_clean) / p_clean),
    ``accuracy`` [n_windows] (share of prompts whose answer token is in the
    knocked top-``topk``), ``clean_prob`` and ``clean_accuracy`` (floats).  The
    causal counterpart of ``head_attention_profile``.  One clean forward + one
    sweep per launch-sized group; a prompt with nothing blocked costs a
    clean re-evaluation."""
    cfg = model.cfg
    prompts, answers = normalize_cie_inputs(model, scrambled_prompts, prompt_answers)
    keys, wins, hs = _check_knockout(cfg, prompts, len(answers), blocked, windows, heads, topk)
    dev, n_win, n_prompts = model.device, len(wins), len(prompts)
    dsum = torch.zeros(n_win, device=dev)
    rsum = torch.zeros(n_win, device=dev)
    hits = torch.zeros(n_win, device=dev)
    clean_p = clean_hits = 0.0
    # one window's members, (layer, head, vec ignored)
    members = [np.asarray([(l, h, -1) for l in range(a, b + 1) for h in hs], dtype=np.int32).reshape(-1, 3)
               for a, b in wins]
    win_chunk = max(1, min(n_win, MAX_SITES_PER_LAUNCH))
    group = max(1, MAX_SITES_PER_LAUNCH // win_chunk)
    for a, b in _chunks(n_prompts, group):
        seqs = [list(map(int, p)) for p in prompts[a:b]]
        tg = np.asarray(answers[a:b], dtype=np.int32)
        n = len(seqs)
        trace = model._sweep_trace(n, sum(len(s) for s in seqs))
        clean = model.forward_clean(seqs, targets=tg.tolist(), topk=topk, trace=trace, defer=n_win > 0)
        tgd = torch.as_tensor(tg, device=dev)
        for wa, wb in _chunks(n_win, win_chunk):
            m = wb - wa
            sites = make_sites(n * m)
            sites["seq"] = np.repeat(np.arange(n, dtype=np.int32), m)
            sites["kind"] = _lib.SITE_ATTN_KNOCKOUT_LASTPOS
            sites["target"] = np.repeat(tg, m)
            sizes = np.tile([len(x) for x in members[wa:wb]], n)
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
            pat = np.tile(np.concatenate(members[wa:wb]), (n, 1))
            ksizes = np.repeat([len(k) for k in keys[a:b]], m)
            koff = np.concatenate([[0], np.cumsum(ksizes)]).astype(np.int32)
            kk = np.asarray([j for k in keys[a:b] for _ in range(m) for j in k], dtype=np.int32)
            out = model.patch_sweep_knockout(trace, sites, off, pat, koff, kk, topk=topk)
            p = out["prob"].view(n, m)
            diff = p - clean["prob"][:, None]
            dsum[wa:wb] += diff.sum(0)
            rsum[wa:wb] += (diff / clean["prob"][:, None]).sum(0)
            hits[wa:wb] += (out["topk"].view(n, m, topk) == tgd[:, None, None]).any(-1).sum(0)
        # (the deferred clean outputs are written by the group's first sweep; without windows the forward ran at once)
        clean_p += float(clean["prob"].sum())
        clean_hits += float((clean["topk"] == tgd[:, None]).any(-1).sum())
    return {"dprob": dsum / n_prompts, "rel_dprob": rsum / n_prompts, "accuracy": hits / n_prompts,
            "clean_prob": clean_p / n_prompts, "clean_accuracy": clean_hits / n_prompts}


def knockout_role_prompts(model, contexts: Pairs, function_token: str, seperator_token: Optional[str],
                          num_contexts: int, len_contexts: int):
    """``sample_icl_prompts_with_roles`` and the first token of each query
    pair's label: (prompts, roles, answers).  The labels come from a replay of
    the same shuffles; the global ``random`` ends where the sampler left it."""
    state = random.getstate()
    prompts, roles = sample_icl_prompts_with_roles(model, contexts, function_token, seperator_token, num_contexts,
                                                   len_contexts)
    end = random.getstate()
    random.setstate(state)
    pool, answers = list(contexts), []
    for _ in range(num_contexts):
        random.shuffle(pool)
        answers.append(int(model.tokenizer.encode(pool[len_contexts][1])[0]))
    random.setstate(end)
    return prompts, roles, answers


@range_checked
def head_source_attribution(contexts: Pairs, function_token: str, seperator_token: Optional[str] = None,
                            model: Model = None, num_contexts: int = 256, len_contexts: int = 4,
                            contrast_answers=None) -> torch.Tensor:
    """FROM WHICH tokens every head carries the answer's logit: the mean over
    ``num_contexts`` prompts (``knockout_role_prompts``: the prompt stream of
    ``head_attention_profile``, the answer the first token of the query pair's
    label) of each head's direct logit attribution at the last position, split
    over the roles of ``prompts.ROLES`` of the keys it attends to.
    [n_layers, n_heads, len(ROLES)] on the device; its sum over the roles is
    ``head_logit_attribution(prompts, answers).heads`` on the same prompts.  A
    head can spread its attention over the demonstrations' labels and take all
    of its push from one of them, or attend to BOS with a value that writes
    nothing along the answer: ``head_attention_profile`` says where a head
    looks, this what it brings back from there.  ``contrast_answers`` (one per
    prompt, in ``head_logit_attribution``'s forms) attributes the logit difference.  One clean
    forward into a trace and one pass over its Q / K / V rows
    (``Trace.source_attribution``) per ``EXTRACT_BATCH`` prompts, no patched
    forward."""
    if num_contexts <= 0:
        raise ValueError("num_contexts must be positive")
    if len_contexts < 0 or len_contexts >= len(contexts):
        raise ValueError("len_contexts must be smaller than the number of contexts (demos + one query)")
    if contrast_answers is not None and len(contrast_answers) != num_contexts:
        raise ValueError("Contrast answers must be of the same length as the prompts (num_contexts)")
    prompts, roles, answers = knockout_role_prompts(model, contexts, function_token, seperator_token, num_contexts,
                                                    len_contexts)
    contrast = normalize_cie_inputs(model, [], contrast_answers)[1] if contrast_answers is not None else None
    total = None
    for a, b in _chunks(len(prompts), EXTRACT_BATCH):
        seqs = prompts[a:b]
        trace = model._sweep_trace(len(seqs), sum(len(s) for s in seqs))
        model.forward_clean(seqs, trace=trace)
        part = trace.source_attribution(answers[a:b], contrast=contrast[a:b] if contrast is not None else None,
                                        classes=roles[a:b], n_classes=len(ROLES))[1].sum(0)  # prompts in order
        total = part if total is None else total + part
    return total / num_contexts


def top_source_heads(profile: torch.Tensor, role, num_heads: int) -> List[Tuple[int, int]]:
    """The ``num_heads`` (layer, head) pairs of a ``head_source_attribution``
    that carry the most attribution from ``role`` (a name of ``prompts.ROLES``
    or its index), highest first (torch.topk's order and tie rule, as
    ``top_attention_heads``)."""
    return top_attention_heads(profile, role, num_heads)


@range_checked
def attention_knockout_by_role(contexts: Pairs, function_token: str, seperator_token: Optional[str] = None,
                               model: Model = None, num_contexts: int = 64, len_contexts: int = 4,
                               roles: Sequence[str] = ROLES[:-1], window: Optional[int] = None, stride: int = 1,
                               topk: int = 1) -> dict:
    """Does the prediction DEPEND on where the last token looks?  For every
    role of ``roles`` (names of ``prompts.ROLES``) and every window of
    ``window`` consecutive layers (default ``max(1, n_layers // 4)``), stepped
    by ``stride``, block the last token's attention to all tokens of that role
    in all heads of the window and re-measure the first token of the query
    pair's label, over ``num_contexts`` prompts of
    ``sample_icl_prompts_with_roles`` (``head_attention_profile``'s stream).
    Returns ``roles``, ``windows`` ((first, last) inclusive), ``dprob`` /
    ``rel_dprob`` / ``accuracy`` [n_roles, n_windows] (device) and
    ``clean_prob`` / ``clean_accuracy``.  A role a prompt does not contain
    leaves that prompt unchanged (an empty key list)."""
    cfg = model.cfg
    if num_contexts <= 0:
        raise ValueError("num_contexts must be positive")
    if len_contexts < 0 or len_contexts >= len(contexts):
        raise ValueError("len_contexts must be smaller than the number of contexts (demos + one query)")
    roles = [str(r) for r in roles]
    if not roles or any(r not in ROLES for r in roles):
        raise ValueError(f"roles must be names of {ROLES}")
    window = max(1, cfg.n_layers // 4) if window is None else int(window)
    if not 1 <= window <= cfg.n_layers or stride < 1:
        raise ValueError("window must be in [1, n_layers] and stride at least 1")
    windows = [(a, a + window - 1) for a in range(0, cfg.n_layers - window + 1, stride)]
    prompts, token_roles, answers = knockout_role_prompts(model, contexts, function_token, seperator_token,
                                                          num_contexts, len_contexts)
    out = {"roles": roles, "windows": windows}
    rows = {"dprob": [], "rel_dprob": [], "accuracy": []}
    for r in roles:
        idx = ROLES.index(r)
        blocked = [[j for j, c in enumerate(tr) if c == idx] for tr in token_roles]
        res = attention_knockout_effect(prompts, answers, blocked, windows, model=model, topk=topk)
        for k in rows:
            rows[k].append(res[k])
        out["clean_prob"], out["clean_accuracy"] = res["clean_prob"], res["clean_accuracy"]
    for k in rows:
        out[k] = torch.stack(rows[k])
    return out
