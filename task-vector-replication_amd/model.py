"""``Model``: the handle the façade passes where the reference passes a
TransformerLens ``HookedTransformer`` (scratch2.py:26 and every ``model=``
argument).  It owns the processed device weights, exposes ``cfg`` and the
token helpers, and drives the engine's batched entry points:

* ``forward_clean``  — many prompts in one launch sequence (replaces the
  per-prompt ``forward`` / ``run_with_cache`` calls);
* ``patch_sweep``    — many (prompt, patch site) pairs in one staircase
  launch sequence (replaces the per-site ``run_with_hooks`` loops);
* ``project_heads``  — z-form capture → ``hook_result`` form;
* ``capture_resid``  — grouped sums of ``hook_resid_pre`` rows of a trace, every
  layer at once (replaces ``run_with_cache`` + a Python mean over prompts);
* ``logit_attribution`` / ``head_attribution`` — every head's and every layer's
  push on a token's logit from a trace (``stack_head_results`` + ``logit_attrs``);
* ``source_attribution`` / ``head_directions`` — every head's push split over the
  key tokens it attends to (pattern × value-weighted attribution, per key or per
  class of keys);
* ``logit_lens`` / ``decode_rows`` — residual rows of every layer, or any
  vectors, through the final LayerNorm and the unembedding.

The compute entry points run as torch.library operators (``torch.ops.tvr.*``,
csrc/torch_ops.cpp over the C ABI) on torch's current stream, with outputs
from torch's allocator; nothing here has a CPU fallback (the engine refuses to
run without a GPU).

The x2f16 range check (include/tvr.h ``tvr_model_range_status``) reads a
device-side sticky flag and synchronises: a direct call checks after itself,
an experiment function (``range_checked``) once at its end, so its sweeps
enqueue back to back.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import inspect
import random
import warnings
import weakref
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .config import CConfig, PythiaConfig, get_config
from .tokenizer import HFTokenizer, SyntheticTokenizer, TokenizerMixin
from .weights import (EngineWeights, config_from_hf_json, load_hf_safetensors, process_to_engine,
                      synth_engine_weights)

SITE_DTYPE = np.dtype([(f, np.int32) for f in _lib.SITE_FIELDS])


def range_checked(fn):
    """Run ``fn`` (an experiment function taking ``model``) inside the model's
    range scope: the x2f16 range flag is read once when the outermost scope
    ends instead of after every engine call.

    If that check fails (``_lib.RangeError``: a GEMM input reached the fp16
    split's limit, so the call's results are not fp32-accurate), the model
    moves to the next path without that limit (``Model.range_fallback``:
    the processed-weight GEMMs when the exact-fp16 ones were bound — their A
    operand is LNPre(x)·γ — else gemm ``"x3bf16"``), warns, records it in
    ``model.range_fallbacks``, restores the global ``random`` state the call
    started from and runs the call again: same process, same prompts (the
    functions shuffle private copies of their inputs; substitute_task's
    in-place sort is idempotent)."""
    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        try:
            model = sig.bind_partial(*args, **kwargs).arguments.get("model")
        except TypeError:  # a bad call: let fn raise its own error
            model = None
        if not isinstance(model, Model):
            return fn(*args, **kwargs)
        if model._range_depth > 0 or not model.range_fallback:  # the outermost call retries
            with model.range_scope(fn.__name__):
                return fn(*args, **kwargs)
        state = random.getstate()
        while True:
            try:
                with model.range_scope(fn.__name__):
                    return fn(*args, **kwargs)
            except _lib.RangeError as e:
                if not model._fall_back(fn.__name__, e):
                    raise
                random.setstate(state)
    return wrapper


def make_sites(n: int) -> np.ndarray:
    """Zeroed site records (layout of ``tvr_site``), target = -1."""
    s = np.zeros(n, dtype=SITE_DTYPE)
    s["target"] = -1
    return s


class Trace:
    """Engine-owned clean-run snapshots (resid_pre per layer, z, K/V).

    A caller's trace keeps its model alive; the experiment functions' scratch
    trace (``weak``) does not, so ``del model`` frees the model's device memory
    at once (no model <-> trace reference cycle waiting for the collector).
    The model closes every live trace before it destroys itself."""

    def __init__(self, model: "Model", max_seqs: int, max_tokens: int, weak: bool = False):
        self._lib = model._lib
        self._h = None
        h = ctypes.c_void_p()
        _lib.check(self._lib.tvr_trace_create(model._h, max_seqs, max_tokens, ctypes.byref(h)),
                   "tvr_trace_create")
        self._h = h
        self._model_strong = None if weak else model
        self._model_ref = weakref.ref(model)
        model._traces.add(self)
        self.max_seqs = max_seqs
        self.max_tokens = max_tokens
        self.seq_lens: List[int] = []
        self.seq_offsets: List[int] = []
        # output tensors of a deferred clean forward, kept alive until the
        # engine has written them (the next patch sweep or trace read)
        self._pending_out = None

    @property
    def model(self) -> "Model":
        m = self._model_strong if self._model_strong is not None else self._model_ref()
        if m is None:
            raise _lib.EngineError("the trace's model has been destroyed")
        return m

    def resid_pre(self, layer: int) -> torch.Tensor:
        """``blocks.{layer}.hook_resid_pre`` of every traced token ([tokens, d]);
        layer == n_layers gives the final residual."""
        return self._read(_lib.TRACE_RESID_PRE, layer)

    def z(self, layer: int) -> torch.Tensor:
        """``blocks.{layer}.attn.hook_z`` flattened over heads ([tokens, d])."""
        return self._read(_lib.TRACE_Z, layer)

    def q(self, layer: int) -> torch.Tensor:
        """``blocks.{layer}.attn.hook_q`` flattened over heads ([tokens, d]),
        before rotary (TransformerLens' ``hook_q``, not ``hook_rot_q``)."""
        return self._read(_lib.TRACE_Q, layer)

    def k(self, layer: int) -> torch.Tensor:
        """``blocks.{layer}.attn.hook_k`` flattened over heads ([tokens, d]), before rotary."""
        return self._read(_lib.TRACE_K, layer)

    def v(self, layer: int) -> torch.Tensor:
        """``blocks.{layer}.attn.hook_v`` flattened over heads ([tokens, d]);
        ``b_V`` is zero, as in the processed model (``fold_value_biases``)."""
        return self._read(_lib.TRACE_V, layer)

    def attention_pattern(self, pos: Optional[Sequence[int]] = None) -> torch.Tensor:
        """``blocks.{l}.attn.hook_pattern[0, h, pos[s], :]`` of every traced
        sequence ``s``, layer and head: ``[n_seq, L, H, max(pos) + 1]``, zero
        beyond each sequence's query position.  ``pos`` defaults to every
        sequence's last position.  Replaces one ``run_with_cache`` per prompt
        and ``cache["pattern", l][0, :, -1, :]`` per layer."""
        return self.model.capture_pattern(self, positions=pos, want_pattern=True)[0]

    def attention_mass(self, classes, n_classes: int, pos: Optional[Sequence[int]] = None) -> torch.Tensor:
        """The attention the query position ``pos[s]`` of every traced sequence
        pays to each class of keys: ``[n_seq, L, H, n_classes]`` with
        ``[s, l, h, c] = Σ_{j <= pos[s], classes[s][j] == c} pattern[s, l, h, j]``.
        ``classes``: one id in ``[-1, n_classes)`` per traced token, flat or
        one list per sequence; ``-1`` is counted nowhere."""
        return self.model.capture_pattern(self, positions=pos, classes=classes, n_classes=n_classes)[1]

    def logit_attribution(self, targets, contrast=None, pos: Optional[Sequence[int]] = None):
        """Direct logit attribution at ``pos[s]`` of every traced sequence:
        ``(heads [n_seq, L, H], resid [n_seq, L + 1])``; see ``Model.logit_attribution``."""
        return self.model.logit_attribution(self, targets, contrast=contrast, positions=pos)

    def source_attribution(self, targets, contrast=None, pos: Optional[Sequence[int]] = None, classes=None,
                           n_classes: int = 0, want_keys: bool = False):
        """Every head's direct logit attribution at ``pos[s]`` split over the keys
        it attends to: ``(src [n_seq, L, H, max(pos) + 1] or None,
        by_class [n_seq, L, H, n_classes] or None)``; see ``Model.source_attribution``."""
        return self.model.source_attribution(self, targets, contrast=contrast, positions=pos, classes=classes,
                                             n_classes=n_classes, want_keys=want_keys)

    def logit_lens(self, targets=None, pos: Optional[Sequence[int]] = None, topk: int = 0):
        """Every layer's residual row at ``pos[s]`` decoded through the final
        LayerNorm and the unembedding: ``(prob [n_seq, L + 1] or None,
        topk [n_seq, L + 1, k] or None)``; see ``Model.logit_lens``."""
        return self.model.logit_lens(self, targets=targets, positions=pos, topk=topk)

    def _read(self, what: int, layer: int) -> torch.Tensor:
        m = self.model
        buf = torch.empty(sum(self.seq_lens), m.cfg.d_model, device=m.device)
        _lib.check(self._lib.tvr_trace_read(self._h, what, layer, buf.data_ptr(), m._stream()),
                   "tvr_trace_read")
        self._pending_out = None
        return buf

    def flush(self) -> None:
        """Run a pending deferred clean forward now (its prob / top-k tensors
        are written; include/tvr.h tvr_trace_flush)."""
        if self._pending_out is not None:
            _lib.check(self._lib.tvr_trace_flush(self._h, self.model._stream()), "tvr_trace_flush")
            self._pending_out = None

    def close(self) -> None:
        """Run a pending deferred forward (its outputs are owed to the caller)
        and free the trace; idempotent.  Model.__del__ calls it on every live
        trace of the model first, so no trace outlives its engine model."""
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                if getattr(self, "_pending_out", None) is not None:
                    self.flush()  # (tvr_trace_destroy would also run it)
            finally:  # the device buffers are released even if the flush raised
                self._h = None
                self._lib.tvr_trace_destroy(h)

    def __del__(self):
        self.close()


# Matrix-core path of the GEMMs (Model.set_gemm): the fp32-accurate 2-plane
# fp16 split is the fastest path whose error is at or below the fp32 MFMA's.
DEFAULT_GEMM = "x2f16"


class Model(TokenizerMixin):
    def __init__(self, cfg: PythiaConfig, weights: EngineWeights, tokenizer=None,
                 device: Optional[torch.device] = None, gemm: str = DEFAULT_GEMM):
        self._h = None
        self._traces = weakref.WeakSet()  # live traces of this model (closed before the model is destroyed)
        self._range_depth = 0
        self._lib = _lib.load()
        self._ops = _lib.load_ops()
        dev = torch.device(device) if device is not None else weights.w_embed.device
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise _lib.EngineError("the HIP engine needs a GPU device (no CPU fallback): "
                                   f"got device {dev}")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.cfg = cfg
        self.device = dev
        self.weights = weights
        self.tokenizer = tokenizer if tokenizer is not None else SyntheticTokenizer(cfg.d_vocab)
        for t in weights.tensors():
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("engine weights must be contiguous fp32 tensors on the model device")
        self._cfg_c = CConfig.from_config(cfg)
        self._layers_c = (_lib.CLayerWeights * cfg.n_layers)(
            *[_lib.CLayerWeights(L.w1.data_ptr(), L.b1.data_ptr(), L.w2.data_ptr(), L.b2.data_ptr())
              for L in weights.layers])
        h = ctypes.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(self._lib.tvr_model_create(
                ctypes.byref(self._cfg_c), weights.w_embed.data_ptr(), self._layers_c,
                weights.w_unembed_t.data_ptr(), weights.b_unembed.data_ptr(), ctypes.byref(h)),
                "tvr_model_create")
        self._h = h
        self._trace_cache: Optional[Trace] = None
        self.exact16 = False
        self._x16_c = None
        self.gemm = "f32"
        # what an experiment function does when the x2f16 range check fails (range_checked): retry on the
        # next path without the limit (True), or raise (False); the fallbacks taken, as (function, path)
        self.range_fallback = True
        self.range_fallbacks: List[tuple] = []
        if weights.raw16 is not None:  # bound first: the x2f16 planes are then built without W2's
            self.set_exact16(True)
        self.set_gemm(gemm)

    # ------------------------------------------------------------------ build
    @classmethod
    def from_pretrained(cls, name: str, device="cuda", seed: int = 0, checkpoint: Optional[str] = None,
                        tokenizer_path: Optional[str] = None, std: float = 0.02, ln_std: float = 0.1,
                        cfg: Optional[PythiaConfig] = None, gemm: str = DEFAULT_GEMM,
                        fp16_weights: bool = False) -> "Model":
        """``HookedTransformer.from_pretrained`` without a network: the named
        Pythia shape with seeded synthetic weights (generated on the device), or
        a local HF-layout safetensors ``checkpoint`` (file, or directory with
        model.safetensors / sharded index; its config.json, when present,
        supplies the shape for names this module does not know).  ``gemm``
        picks the matrix-core path (see :meth:`set_gemm`).  ``fp16_weights``:
        the synthetic parameters are fp16-valued, as the released checkpoints
        are; with fp16-valued weights (synthetic or a checkpoint's) the
        exact-fp16 GEMMs are bound (:meth:`set_exact16`)."""
        import os
        if cfg is None:
            try:
                cfg = get_config(name)
            except ValueError:
                if not (checkpoint and os.path.isdir(checkpoint)):
                    raise
                cfg = config_from_hf_json(checkpoint)
        dev = torch.device(device)
        if checkpoint:
            w = process_to_engine(cfg, load_hf_safetensors(checkpoint, cfg), device=dev, free_source=True)
        else:
            w = synth_engine_weights(cfg, seed=seed, device=dev, std=std, ln_std=ln_std, fp16=fp16_weights)
        tok = HFTokenizer(tokenizer_path) if tokenizer_path else None
        if dev.type == "cuda":
            torch.cuda.empty_cache()  # the generation's temporaries: the engine's own allocations come next
        return cls(cfg, w, tokenizer=tok, device=dev, gemm=gemm)

    @classmethod
    def from_hf_state_dict(cls, cfg: PythiaConfig, sd, device="cuda", tokenizer=None,
                           gemm: str = DEFAULT_GEMM) -> "Model":
        return cls(cfg, process_to_engine(cfg, sd, device=torch.device(device)), tokenizer, device, gemm)

    def set_gemm(self, mode: str) -> None:
        """Matrix-core path of every GEMM (include/tvr.h ``tvr_model_set_gemm``):
        ``"x2f16"`` (default) — fp32-accurate two-plane fp16 split (the fp16 form
        of 3xTF32: three products on the fp16 MFMA, 4 B per weight for the
        planes; inputs must stay below 4095 in magnitude, checked on the device
        after every engine call); ``"x3bf16"`` — fp32-accurate three-plane bf16
        split (six products, 6 B per weight, no range limit); ``"f32"`` —
        ``v_mfma_f32_32x32x2_f32`` on the fp32 weights; ``"bf16"`` — bf16
        weights and GEMM inputs, fp32 accumulation (NOT fp32-accurate: the
        north star's bf16 configuration, 2e-2 tolerance).  Both splits measure
        at or below the fp32 MFMA GEMM's error against fp64 (DESIGN.md
        section 3).  Everything outside the GEMMs is fp32 in all four."""
        if mode not in _lib.GEMM_MODES:
            raise ValueError(f"gemm mode must be one of {sorted(_lib.GEMM_MODES)}, got {mode!r}")
        with torch.cuda.device(self.device):
            try:
                _lib.check(self._lib.tvr_model_set_gemm(self._h, _lib.GEMM_MODES[mode], self._stream()),
                           "tvr_model_set_gemm")
            finally:  # a failed switch leaves the engine in the fp32 mode: mirror it
                self.gemm = _lib.GEMM_NAMES.get(self._lib.tvr_model_get_gemm(self._h), mode)

    def set_exact16(self, on: bool) -> None:
        """Bind (or detach) the checkpoint's own fp16 GEMM weights
        (``EngineWeights.raw16``; include/tvr.h ``tvr_model_set_exact16``): in
        x2f16 mode the QKV + MLP-in and O + MLP-out GEMMs then run 2 matrix
        products per slice instead of 3 on those exact operands, with LN's
        gamma applied to the rows.  On by default whenever the weights are
        fp16-valued (every released Pythia checkpoint).  Results equal the
        processed-weight path's to fp32 rounding."""
        raw = self.weights.raw16
        if on and raw is None:
            raise ValueError("set_exact16: the weights are not exact in fp16 (EngineWeights.raw16 is None)")
        if on:
            for r in raw:
                for t, dt in ((r.w1, torch.float16), (r.w2, torch.float16), (r.g1, torch.float32),
                              (r.g2, torch.float32)):
                    if t.device != self.device or t.dtype != dt or not t.is_contiguous():
                        raise ValueError("raw16 tensors must be contiguous fp16 (w1, w2) / fp32 (g1, g2) on the "
                                         "model device")
            ru = self.weights.raw16_unembed
            if ru is not None:
                wu, gf = ru
                if wu.device != self.device or wu.dtype != torch.float16 or not wu.is_contiguous() or \
                        gf.device != self.device or gf.dtype != torch.float32:
                    raise ValueError("raw16_unembed must be (fp16 [V, d], fp32 [d]) contiguous on the model device")
            arr = (_lib.CExact16Layer * self.cfg.n_layers)(
                *[_lib.CExact16Layer(r.w1.data_ptr(), r.w2.data_ptr(), r.g1.data_ptr(), r.g2.data_ptr())
                  for r in raw])
        # the engine re-plans the x2f16 weight planes on a (de)tach: hipMalloc / the conversion kernels run on
        # the current device, which must be the model's
        with torch.cuda.device(self.device):
            try:
                if on:
                    self._x16_c = arr  # the engine keeps the binding from here on, even if the re-plan fails
                    _lib.check(self._lib.tvr_model_set_exact16(self._h, arr), "tvr_model_set_exact16")
                    if ru is not None:
                        _lib.check(self._lib.tvr_model_set_exact16_unembed(self._h, wu.data_ptr(), gf.data_ptr()),
                                   "tvr_model_set_exact16_unembed")
                else:
                    _lib.check(self._lib.tvr_model_set_exact16_unembed(self._h, None, None),
                               "tvr_model_set_exact16_unembed")
                    _lib.check(self._lib.tvr_model_set_exact16(self._h, None), "tvr_model_set_exact16")
                    self._x16_c = None
            finally:
                # the engine records the binding before it re-plans, and a failed re-plan (e.g. the planes do
                # not fit) leaves it in the fp32 mode: mirror what the engine holds, error or not
                self.exact16 = bool(on)
                self.gemm = _lib.GEMM_NAMES.get(self._lib.tvr_model_get_gemm(self._h), self.gemm)

    @property
    def weight_layout(self) -> int:
        """Which exact-fp16 weights the GEMMs read from the engine's row-pair-interleaved copies (include/tvr.h
        ``tvr_model_weight_layout``): a mask of ``_lib.W_IL_LAYERS`` / ``W_IL_UNEMBED``, with ``W_IL_NOMEM`` when a
        copy did not fit and its GEMMs read the plain plane; 0 off the exact-fp16 path and under
        ``TVR_W_LAYOUT=rows``."""
        return int(self._lib.tvr_model_weight_layout(self._h))

    def _fall_back(self, what: str, err: Exception) -> bool:
        """Move to the next GEMM path without the x2f16 range limit after a
        failed range check: exact-fp16 → processed weights (x2f16, 3 products:
        LayerNorm's output, bounded by sqrt(d_model), is the A operand again),
        x2f16 → x3bf16 (no range limit).  False when there is none left."""
        if self.gemm != "x2f16":
            return False
        if self.exact16:
            self.set_exact16(False)  # the engine re-plans the x2f16 planes on the processed weights
            path = "x2f16 (processed weights)"
        else:
            self.set_gemm("x3bf16")
            path = "x3bf16"
        self.range_fallbacks.append((what, path))
        warnings.warn(f"{what}: {err} -- retrying on {path}", RuntimeWarning, stacklevel=3)
        return True

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            for t in list(getattr(self, "_traces", ())):
                t.close()  # before the engine model they point into is freed
            self._trace_cache = None
            self._h = None
            self._lib.tvr_model_destroy(h)

    # ------------------------------------------------------------- internals
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check_range(self, what: str, force: bool = False) -> None:
        """x2f16 only: fail loudly if a GEMM input left the fp16 split's range
        since the last check (synchronises the stream).  Inside a
        ``range_scope`` the check waits for the scope's end."""
        if self.gemm == "x2f16" and (force or self._range_depth == 0):
            _lib.check(self._lib.tvr_model_range_status(self._h, self._stream()), what)

    @contextlib.contextmanager
    def range_scope(self, what: str):
        """Defer the per-call range checks of the engine calls inside to ONE
        check when the outermost scope exits normally (the flag is sticky on
        the device, so nothing is missed; an exception propagates unchecked)."""
        self._range_depth += 1
        try:
            yield self
        except BaseException:
            self._range_depth -= 1
            raise
        self._range_depth -= 1
        self._check_range(what)

    def _op(self, name: str, *args):
        """torch.ops.tvr.<name>: engine errors as EngineError (invalid
        arguments stay ValueError, the reference's error type)."""
        try:
            return getattr(self._ops, name)(*args)
        except ValueError:
            raise
        except RuntimeError as e:
            raise _lib.EngineError(str(e)) from e

    def trace(self, n_seqs: int, n_tokens: int) -> Trace:
        """A new trace with this capacity, owned by the caller (the experiment
        functions use a private one, so they never overwrite it)."""
        return Trace(self, max(n_seqs, 1), max(n_tokens, 1))

    def _sweep_trace(self, n_seqs: int, n_tokens: int) -> Trace:
        """The experiment functions' scratch trace (grown on demand, reused)."""
        t = self._trace_cache
        if t is None or t.max_seqs < n_seqs or t.max_tokens < n_tokens:
            if t is not None:
                t.flush()  # a deferral on the old trace still owes its outputs
            self._trace_cache = None
            t = Trace(self, max(n_seqs, 1), max(n_tokens, 1), weak=True)
            self._trace_cache = t
        return t

    @staticmethod
    def _pack(seqs: Sequence[Sequence[int]]):
        lens = np.asarray([len(s) for s in seqs], dtype=np.int32)
        toks = np.asarray([int(x) for s in seqs for x in s], dtype=np.int32)
        return toks, lens

    # ---------------------------------------------------------- entry points
    def forward_clean(self, seqs: Sequence[Sequence[int]], targets: Optional[Sequence[int]] = None,
                      topk: int = 0, return_logits: bool = False, capture: bool = False,
                      trace: Optional[Trace] = None, defer: bool = False) -> Dict[str, torch.Tensor]:
        """Batched clean forward of ragged prompts (token-id lists).
        Returns ``prob`` [n] (softmax(logits[-1])[target]), ``topk`` [n, k],
        ``logits`` [n, V] (last position), ``zsum`` [L, d] (sum over prompts of
        hook_z at the last position) as requested.
        ``defer`` (with a trace; no logits / capture): the clean rows run inside
        the next ``patch_sweep`` on that trace (tvr_forward_clean_deferred) and
        the returned tensors are written by it — read them after that sweep."""
        n = len(seqs)
        if n == 0:
            raise ValueError("no prompts")
        toks, lens = self._pack(seqs)
        tg = None
        if targets is not None:
            tg = np.asarray([-1 if t is None else int(t) for t in targets], dtype=np.int32)
            if tg.shape[0] != n:
                raise ValueError("targets must have one entry per prompt")
        if trace is not None and (trace.max_seqs < n or trace.max_tokens < int(lens.sum())):
            raise ValueError("trace too small for this batch")
        if defer and (trace is None or return_logits or capture):
            raise ValueError("defer needs a trace and no logits / capture")
        cfg = self.cfg
        prob, top, logits, zsum = self._op(
            "forward_clean", self._h.value, trace._h.value if trace is not None else 0, torch.from_numpy(toks),
            torch.from_numpy(lens), torch.from_numpy(tg) if tg is not None else None, topk, return_logits, capture,
            defer, cfg.n_layers, cfg.d_model, cfg.d_vocab, self.device)
        out = {}
        if tg is not None:
            out["prob"] = prob
        if topk:
            out["topk"] = top
        if return_logits:
            out["logits"] = logits
        if capture:
            out["zsum"] = zsum
        if trace is not None:
            trace.seq_lens = lens.tolist()
            trace.seq_offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
            # a deferred forward's outputs are written by the next sweep on the trace: keep them alive
            trace._pending_out = (prob, top) if defer else None
        if not defer:
            self._check_range("tvr_forward_clean")
        return out

    def patch_sweep(self, trace: Trace, sites: np.ndarray, vectors: Optional[torch.Tensor] = None,
                    topk: int = 0, want_prob: bool = True, return_logits: bool = False
                    ) -> Dict[str, torch.Tensor]:
        """Evaluate every site (records of ``make_sites``) against ``trace``."""
        sites = np.ascontiguousarray(sites, dtype=SITE_DTYPE)
        n = int(sites.shape[0])
        if n == 0:
            raise ValueError("no patch sites")
        if vectors is not None:
            if vectors.device != self.device or vectors.dtype != torch.float32:
                raise ValueError("vectors must be fp32 on the model device")
            vectors = vectors.reshape(-1, self.cfg.d_model).contiguous()
        rows = torch.from_numpy(sites.view(np.int32).reshape(n, len(_lib.SITE_FIELDS)))
        prob, top, logits = self._op("patch_sweep", self._h.value, trace._h.value, rows, vectors, topk, want_prob,
                                     return_logits, self.cfg.d_vocab, self.device)
        self._check_range("tvr_patch_sweep")
        trace._pending_out = None
        out = {}
        if want_prob:
            out["prob"] = prob
        if topk:
            out["topk"] = top
        if return_logits:
            out["logits"] = logits
        return out

    def patch_sweep_sets(self, trace: Trace, sites: np.ndarray, set_off, patches,
                         vectors: Optional[torch.Tensor] = None, topk: int = 0, want_prob: bool = True,
                         return_logits: bool = False) -> Dict[str, torch.Tensor]:
        """``patch_sweep`` with joint head-set sites (tvr_patch_sweep_sets): site
        ``i`` of kind ``SITE_REPLACE_HEADSET_ALLPOS`` / ``_LASTPOS`` replaces
        ``hook_result`` of every ``(layer, head)`` of ``patches[set_off[i]:set_off[i+1]]``
        (rows ``(layer, head, vec)``) by ``vectors[vec]``, at every position or at
        the last one; sites of the other kinds own an empty range and behave as
        in ``patch_sweep``.  Returns the same dictionary."""
        sites = np.ascontiguousarray(sites, dtype=SITE_DTYPE)
        n = int(sites.shape[0])
        if n == 0:
            raise ValueError("no patch sites")
        off = np.ascontiguousarray(set_off, dtype=np.int32).reshape(-1)
        pat = np.ascontiguousarray(patches, dtype=np.int32).reshape(-1, 3)
        if off.shape[0] != n + 1:
            raise ValueError("set_off must have n_sites + 1 entries")
        if off[0] < 0 or np.any(np.diff(off) < 0) or off[-1] > pat.shape[0]:
            raise ValueError("set_off must be non-decreasing and stay inside patches")
        if vectors is not None:
            if vectors.device != self.device or vectors.dtype != torch.float32:
                raise ValueError("vectors must be fp32 on the model device")
            vectors = vectors.reshape(-1, self.cfg.d_model).contiguous()
        rows = torch.from_numpy(sites.view(np.int32).reshape(n, len(_lib.SITE_FIELDS)))
        prob, top, logits = self._op("patch_sweep_sets", self._h.value, trace._h.value, rows, torch.from_numpy(off),
                                     torch.from_numpy(pat), vectors, topk, want_prob, return_logits,
                                     self.cfg.d_vocab, self.device)
        self._check_range("tvr_patch_sweep_sets")
        trace._pending_out = None
        out = {}
        if want_prob:
            out["prob"] = prob
        if topk:
            out["topk"] = top
        if return_logits:
            out["logits"] = logits
        return out

    def patch_sweep_knockout(self, trace: Trace, sites: np.ndarray, set_off, patches, key_off, keys,
                             vectors: Optional[torch.Tensor] = None, topk: int = 0, want_prob: bool = True,
                             return_logits: bool = False) -> Dict[str, torch.Tensor]:
        """``patch_sweep_sets`` with attention-knockout sites
        (tvr_patch_sweep_knockout): site ``i`` of kind
        ``SITE_ATTN_KNOCKOUT_LASTPOS`` sets
        ``hook_attn_scores[0, head, -1, j] = -inf`` for every ``(layer, head)``
        of ``patches[set_off[i]:set_off[i+1]]`` (rows ``(layer, head, vec)``,
        ``vec`` ignored) and every key position ``j`` of
        ``keys[key_off[i]:key_off[i+1]]`` (strictly increasing, at least one
        key of the prompt left).  The other kinds own an empty key range and
        behave as in ``patch_sweep_sets``.  Returns the same dictionary."""
        sites = np.ascontiguousarray(sites, dtype=SITE_DTYPE)
        n = int(sites.shape[0])
        if n == 0:
            raise ValueError("no patch sites")
        off = np.ascontiguousarray(set_off, dtype=np.int32).reshape(-1)
        pat = np.ascontiguousarray(patches, dtype=np.int32).reshape(-1, 3)
        koff = np.ascontiguousarray(key_off, dtype=np.int32).reshape(-1)
        kk = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1)
        if off.shape[0] != n + 1 or koff.shape[0] != n + 1:
            raise ValueError("set_off and key_off must have n_sites + 1 entries")
        if off[0] < 0 or np.any(np.diff(off) < 0) or off[-1] > pat.shape[0]:
            raise ValueError("set_off must be non-decreasing and stay inside patches")
        if koff[0] < 0 or np.any(np.diff(koff) < 0) or koff[-1] > kk.shape[0]:
            raise ValueError("key_off must be non-decreasing and stay inside keys")
        if vectors is not None:
            if vectors.device != self.device or vectors.dtype != torch.float32:
                raise ValueError("vectors must be fp32 on the model device")
            vectors = vectors.reshape(-1, self.cfg.d_model).contiguous()
        rows = torch.from_numpy(sites.view(np.int32).reshape(n, len(_lib.SITE_FIELDS)))
        prob, top, logits = self._op("patch_sweep_knockout", self._h.value, trace._h.value, rows,
                                     torch.from_numpy(off), torch.from_numpy(pat), torch.from_numpy(koff),
                                     torch.from_numpy(kk), vectors, topk, want_prob, return_logits,
                                     self.cfg.d_vocab, self.device)
        self._check_range("tvr_patch_sweep_knockout")
        trace._pending_out = None
        out = {}
        if want_prob:
            out["prob"] = prob
        if topk:
            out["topk"] = top
        if return_logits:
            out["logits"] = logits
        return out

    def capture_resid(self, trace: Trace, positions: Optional[Sequence[int]] = None,
                      groups: Optional[Sequence[int]] = None, n_groups: int = 1,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Grouped sums of residual-stream rows of ``trace``
        (tvr_trace_capture_resid): ``[n_groups, L + 1, d]`` with
        ``[g, l] = Σ_{s: groups[s] == g} blocks.{l}.hook_resid_pre[s][positions[s]]``
        (row ``L``: the final residual), TransformerLens' centred values.
        ``positions`` defaults to every sequence's last position, ``groups`` to
        one group; ``groups = range(n)`` with ``n_groups = n`` gives per-prompt
        vectors.  Returns a fresh zeroed tensor with the sums, or ``out``
        (contiguous fp32 on the model device, that shape) with the sums ADDED
        to it.  Bitwise reproducible for a given trace."""
        if trace.model is not self:
            raise ValueError("trace belongs to another model")
        n = len(trace.seq_lens)
        if n == 0:
            raise ValueError("trace is empty: run forward_clean(trace=...) first")
        n_groups = int(n_groups)
        if n_groups <= 0:
            raise ValueError("n_groups must be positive")
        pos = grp = None
        if positions is not None:
            pos = np.ascontiguousarray(positions, dtype=np.int32).reshape(-1)
            if pos.shape[0] != n:
                raise ValueError("positions must have one entry per traced sequence")
            if np.any(pos < 0) or np.any(pos >= np.asarray(trace.seq_lens)):
                raise ValueError("a position lies outside its sequence")
        if groups is not None:
            grp = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
            if grp.shape[0] != n:
                raise ValueError("groups must have one entry per traced sequence")
            if np.any(grp < 0) or np.any(grp >= n_groups):
                raise ValueError("a group lies outside [0, n_groups)")
        shape = (n_groups, self.cfg.n_layers + 1, self.cfg.d_model)
        if out is None:
            out = torch.zeros(shape, device=self.device)
        elif (tuple(out.shape) != shape or out.device != self.device or out.dtype != torch.float32
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous fp32 tensor {shape} on the model device")
        self._op("capture_resid", trace._h.value, torch.from_numpy(pos) if pos is not None else None,
                 torch.from_numpy(grp) if grp is not None else None, n_groups, n, out)
        self._check_range("tvr_trace_capture_resid")  # (a deferred clean forward may have run)
        trace._pending_out = None
        return out

    def capture_pattern(self, trace: Trace, positions: Optional[Sequence[int]] = None, classes=None,
                        n_classes: int = 0, want_pattern: bool = False):
        """One query's attention pattern per traced sequence, every layer and
        head, from the Q / K rows ``trace`` holds (tvr_trace_capture_pattern):
        ``(pattern, mass)`` with ``pattern`` ``[n_seq, L, H, max(positions) + 1]``
        (``want_pattern``, else ``None``) and ``mass`` ``[n_seq, L, H, n_classes]``
        (``classes`` given, else ``None``); see ``Trace.attention_pattern`` and
        ``Trace.attention_mass``.  Every argument is checked before the engine
        is called.  Bitwise reproducible for a given trace."""
        if trace.model is not self:
            raise ValueError("trace belongs to another model")
        lens = np.asarray(trace.seq_lens, dtype=np.int64)
        n = int(lens.shape[0])
        if n == 0:
            raise ValueError("trace is empty: run forward_clean(trace=...) first")
        if not want_pattern and classes is None:
            raise ValueError("nothing to capture: ask for the pattern or give classes")
        pos = None
        if positions is not None:
            pos = np.ascontiguousarray(positions, dtype=np.int32).reshape(-1)
            if pos.shape[0] != n:
                raise ValueError("positions must have one entry per traced sequence")
            if np.any(pos < 0) or np.any(pos >= lens):
                raise ValueError("a position lies outside its sequence")
        cls = None
        if classes is not None:
            n_classes = int(n_classes)
            if not 0 < n_classes <= _lib.PATTERN_MAX_CLASSES:
                raise ValueError(f"n_classes must be in [1, {_lib.PATTERN_MAX_CLASSES}]")
            if len(classes) == n and all(not np.isscalar(c) for c in classes):  # one list per sequence
                if any(len(c) != t for c, t in zip(classes, lens)):
                    raise ValueError("classes must have one entry per traced token")
                classes = [x for c in classes for x in c]
            cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1)
            if cls.shape[0] != int(lens.sum()):
                raise ValueError("classes must have one entry per traced token")
            if np.any(cls < -1) or np.any(cls >= n_classes):
                raise ValueError("a class lies outside [-1, n_classes)")
        cfg = self.cfg
        ld = int(pos.max() if pos is not None else lens.max() - 1) + 1
        pattern = torch.empty(n, cfg.n_layers, cfg.n_heads, ld, device=self.device) if want_pattern else None
        mass = torch.empty(n, cfg.n_layers, cfg.n_heads, n_classes, device=self.device) if cls is not None else None
        self._op("capture_pattern", trace._h.value, torch.from_numpy(pos) if pos is not None else None,
                 torch.from_numpy(cls) if cls is not None else None, n_classes if cls is not None else 0, n,
                 cfg.n_layers, cfg.n_heads, pattern, mass)
        self._check_range("tvr_trace_capture_pattern")  # (a deferred clean forward may have run)
        trace._pending_out = None
        return pattern, mass

    # ------------------------------------------- logit attribution and logit lens
    def _trace_queries(self, trace: Trace, positions):
        """The checks the trace readers below share: (n_seq, pos int32 [n] or None)."""
        if trace.model is not self:
            raise ValueError("trace belongs to another model")
        lens = np.asarray(trace.seq_lens, dtype=np.int64)
        n = int(lens.shape[0])
        if n == 0:
            raise ValueError("trace is empty: run forward_clean(trace=...) first")
        pos = None
        if positions is not None:
            pos = np.ascontiguousarray(positions, dtype=np.int32).reshape(-1)
            if pos.shape[0] != n:
                raise ValueError("positions must have one entry per traced sequence")
            if np.any(pos < 0) or np.any(pos >= lens):
                raise ValueError("a position lies outside its sequence")
        return n, pos

    def _token_ids(self, ids, n: int, name: str) -> np.ndarray:
        a = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if a.shape[0] != n:
            raise ValueError(f"{name} must have one entry per row")
        if np.any(a < 0) or np.any(a >= self.cfg.d_vocab):
            raise ValueError(f"a token of {name} lies outside [0, d_vocab)")
        return a.astype(np.int32)

    @staticmethod
    def _check_topk(topk: int) -> int:
        topk = int(topk)
        if not 0 <= topk <= _lib.STATS_MAX_K:
            raise ValueError(f"topk must be in [0, {_lib.STATS_MAX_K}]")
        return topk

    def head_attribution(self, layer: int, z: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
        """How far each head of ``layer`` writes along a direction
        (tvr_head_attribution): ``out[i, h] = (z[i, h·dh:(h+1)·dh] @ W_O[layer, h]) · dirs[i]``
        for ``z``, ``dirs`` ``[n, d_model]`` (fp32 on the model device), ``[n, n_heads]``.
        W_O is the processed fp32 weight ``project_heads`` reads.  The bits of a
        row depend on that row alone."""
        cfg = self.cfg
        if not 0 <= int(layer) < cfg.n_layers:
            raise ValueError("layer out of range")
        for t, name in ((z, "z"), (dirs, "dirs")):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != cfg.d_model or t.shape[0] == 0:
                raise ValueError(f"{name} must be a tensor [n, d_model]")
            if t.device != self.device or t.dtype != torch.float32:
                raise ValueError(f"{name} must be fp32 on the model device")
        if z.shape[0] != dirs.shape[0]:
            raise ValueError("z and dirs must have the same number of rows")
        z, dirs = z.contiguous(), dirs.contiguous()
        if z.data_ptr() % 16:
            z = z.clone()
        if dirs.data_ptr() % 16:
            dirs = dirs.clone()
        out = torch.empty(z.shape[0], cfg.n_heads, device=self.device)
        self._op("head_attribution", self._h.value, int(layer), z, dirs, cfg.d_model, cfg.n_heads, out)
        return out

    def logit_attribution(self, trace: Trace, targets, contrast=None, positions: Optional[Sequence[int]] = None):
        """Direct logit attribution at one query position per traced sequence
        (tvr_trace_logit_attribution): ``(heads [n, L, H], resid [n, L + 1])``.
        With ``u = W_U[:, target] − W_U[:, contrast]`` (processed weights; no
        ``contrast``: the target's column) and the final LayerNorm's scale σ of
        the query row, ``heads[s, l, h] = hook_result[l][q, h] · u / σ`` and
        ``resid[s, l] = hook_resid_pre[l][q] · u / σ`` (``l = L``: the final
        residual, i.e. logit[target] − logit[contrast] minus the same difference
        of ``b_U``; ``l = 0``: the embedding's share).  TransformerLens:
        ``cache.stack_head_results`` / ``accumulated_resid`` with
        ``apply_ln=True`` under ``logit_attrs``.  ``positions`` defaults to every
        sequence's last position.  Bitwise reproducible for a given trace."""
        n, pos = self._trace_queries(trace, positions)
        tg = self._token_ids(targets, n, "targets")
        ct = self._token_ids(contrast, n, "contrast") if contrast is not None else None
        cfg = self.cfg
        heads = torch.empty(n, cfg.n_layers, cfg.n_heads, device=self.device)
        resid = torch.empty(n, cfg.n_layers + 1, device=self.device)
        self._op("logit_attribution", trace._h.value, torch.from_numpy(pos) if pos is not None else None,
                 torch.from_numpy(tg), torch.from_numpy(ct) if ct is not None else None, n, cfg.n_layers,
                 cfg.n_heads, heads, resid)
        self._check_range("tvr_trace_logit_attribution")  # (a deferred clean forward may have run)
        trace._pending_out = None
        return heads, resid

    def head_directions(self, layer: int, dirs: torch.Tensor) -> torch.Tensor:
        """Directions pulled back through ``W_O`` of ``layer`` into the heads'
        ``z`` coordinates (tvr_head_directions): ``g[i] = dirs[i] @ W_O[layer]ᵀ``
        in ``hook_z``'s flattened (head, d_head) order, so that
        ``(z[h] @ W_O[layer, h]) · dirs[i] = z[h] · g[i, h·dh:(h+1)·dh]`` for any
        ``z``.  ``dirs`` ``[n, d_model]`` fp32 on the model device; ``[n, d_model]``.
        The bits of a row depend on that row alone."""
        cfg = self.cfg
        if not 0 <= int(layer) < cfg.n_layers:
            raise ValueError("layer out of range")
        if not isinstance(dirs, torch.Tensor) or dirs.dim() != 2 or dirs.shape[1] != cfg.d_model or dirs.shape[0] == 0:
            raise ValueError("dirs must be a tensor [n, d_model]")
        if dirs.device != self.device or dirs.dtype != torch.float32:
            raise ValueError("dirs must be fp32 on the model device")
        dirs = dirs.contiguous()
        if dirs.data_ptr() % 16:
            dirs = dirs.clone()
        out = torch.empty(dirs.shape[0], cfg.d_model, device=self.device)
        self._op("head_directions", self._h.value, int(layer), dirs, cfg.d_model, out)
        return out

    @staticmethod
    def _key_classes(classes, n_classes: int, lens: np.ndarray) -> np.ndarray:
        """``capture_pattern``'s class checks: int32 [traced tokens] from a flat
        list or one list per sequence, every id in ``[-1, n_classes)``."""
        n = int(lens.shape[0])
        if not 0 < n_classes <= _lib.PATTERN_MAX_CLASSES:
            raise ValueError(f"n_classes must be in [1, {_lib.PATTERN_MAX_CLASSES}]")
        if len(classes) == n and all(not np.isscalar(c) for c in classes):  # one list per sequence
            if any(len(c) != t for c, t in zip(classes, lens)):
                raise ValueError("classes must have one entry per traced token")
            classes = [x for c in classes for x in c]
        cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1)
        if cls.shape[0] != int(lens.sum()):
            raise ValueError("classes must have one entry per traced token")
        if np.any(cls < -1) or np.any(cls >= n_classes):
            raise ValueError("a class lies outside [-1, n_classes)")
        return cls

    def source_attribution(self, trace: Trace, targets, contrast=None, positions: Optional[Sequence[int]] = None,
                           classes=None, n_classes: int = 0, want_keys: bool = False):
        """From which key tokens every head carries the answer's logit
        (tvr_trace_source_attribution): ``(src, by_class)`` with ``src``
        ``[n, L, H, max(positions) + 1]`` (``want_keys``, else ``None``),
        ``src[s, l, h, j] = pattern[l][h, q, j] · ((hook_v[l][j, h] @ W_O[l, h]) · u / σ)``
        for the keys ``j ≤ q`` and zero beyond, and ``by_class``
        ``[n, L, H, n_classes]`` (``classes`` given, else ``None``) its sums over
        the keys of each class.  ``u``, σ, ``targets``, ``contrast`` and
        ``positions`` as in ``logit_attribution``, whose ``heads`` are the sums of
        ``src`` over the keys (``b_V`` is zero in the processed model);
        ``classes`` as in ``Trace.attention_mass``.  Every argument is checked
        before the engine is called.  Bitwise reproducible for a given trace."""
        n, pos = self._trace_queries(trace, positions)
        tg = self._token_ids(targets, n, "targets")
        ct = self._token_ids(contrast, n, "contrast") if contrast is not None else None
        if not want_keys and classes is None:
            raise ValueError("nothing to attribute: ask for the keys or give classes")
        lens = np.asarray(trace.seq_lens, dtype=np.int64)
        cls = None
        if classes is not None:
            n_classes = int(n_classes)
            cls = Model._key_classes(classes, n_classes, lens)
        cfg = self.cfg
        ld = int(pos.max() if pos is not None else lens.max() - 1) + 1
        src = torch.empty(n, cfg.n_layers, cfg.n_heads, ld, device=self.device) if want_keys else None
        by_class = torch.empty(n, cfg.n_layers, cfg.n_heads, n_classes, device=self.device) if cls is not None else None
        self._op("source_attribution", trace._h.value, torch.from_numpy(pos) if pos is not None else None,
                 torch.from_numpy(tg), torch.from_numpy(ct) if ct is not None else None,
                 torch.from_numpy(cls) if cls is not None else None, n_classes if cls is not None else 0, n,
                 cfg.n_layers, cfg.n_heads, src, by_class)
        self._check_range("tvr_trace_source_attribution")  # (a deferred clean forward may have run)
        trace._pending_out = None
        return src, by_class

    def logit_lens(self, trace: Trace, targets=None, positions: Optional[Sequence[int]] = None, topk: int = 0):
        """Every layer's residual row at the query position through the final
        LayerNorm and the unembedding (tvr_trace_logit_lens): ``(prob, topk)``
        with ``prob`` ``[n, L + 1]`` = softmax(logits)[target] (``targets``
        given, else ``None``) and ``topk`` ``[n, L + 1, k]`` int32 token ids
        (``topk > 0``, else ``None``).  Row ``L`` is the model's own
        distribution at the query position."""
        n, pos = self._trace_queries(trace, positions)
        topk = self._check_topk(topk)
        tg = self._token_ids(targets, n, "targets") if targets is not None else None
        if tg is None and topk == 0:
            raise ValueError("nothing to decode: give targets or topk > 0")
        L = self.cfg.n_layers
        prob = torch.empty(n, L + 1, device=self.device) if tg is not None else None
        top = torch.empty(n, L + 1, topk, dtype=torch.int32, device=self.device) if topk else None
        self._op("logit_lens", trace._h.value, torch.from_numpy(pos) if pos is not None else None,
                 torch.from_numpy(tg) if tg is not None else None, n, L, topk, prob, top)
        self._check_range("tvr_trace_logit_lens")
        trace._pending_out = None
        return prob, top

    def decode_rows(self, rows: torch.Tensor, targets=None, topk: int = 0):
        """Decode any vectors ``[n, d_model]`` (task vectors, function vectors,
        residual rows) through the final LayerNorm and the unembedding
        (tvr_decode_rows): ``(prob [n] or None, topk [n, k] int32 or None)``."""
        if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[1] != self.cfg.d_model or \
                rows.shape[0] == 0:
            raise ValueError("rows must be a tensor [n, d_model]")
        if rows.device != self.device or rows.dtype != torch.float32:
            raise ValueError("rows must be fp32 on the model device")
        n = int(rows.shape[0])
        topk = self._check_topk(topk)
        tg = self._token_ids(targets, n, "targets") if targets is not None else None
        if tg is None and topk == 0:
            raise ValueError("nothing to decode: give targets or topk > 0")
        rows = rows.contiguous()
        if rows.data_ptr() % 16:
            rows = rows.clone()
        prob = torch.empty(n, device=self.device) if tg is not None else None
        top = torch.empty(n, topk, dtype=torch.int32, device=self.device) if topk else None
        self._op("decode_rows", self._h.value, rows, torch.from_numpy(tg) if tg is not None else None, topk,
                 self.cfg.d_model, prob, top)
        self._check_range("tvr_decode_rows")
        return prob, top

    def project_heads(self, zsum: torch.Tensor) -> torch.Tensor:
        """[L, d] z-sums → [L, H, d] hook_result sums."""
        if tuple(zsum.shape) != (self.cfg.n_layers, self.cfg.d_model):
            raise ValueError("zsum must be [n_layers, d_model]")
        return self._op("project_heads", self._h.value, zsum.to(self.device, torch.float32).contiguous(),
                        self.cfg.n_heads)

    # ------------------------------------------------------------ profiling
    def profile(self, on: bool) -> None:
        """Enable/disable HIP-event timing of every GEMM and HBM-bound kernel launch (resets totals)."""
        _lib.check(self._lib.tvr_profile_enable(self._h, 1 if on else 0), "tvr_profile_enable")

    def profile_stats(self) -> dict:
        st = _lib.CKernelStats()
        _lib.check(self._lib.tvr_profile_read(self._h, ctypes.byref(st)), "tvr_profile_read")
        per = {name: {"launches": st.gemm_launches[i], "flops": st.gemm_flops[i], "ms": st.gemm_ms[i],
                      "bytes": st.gemm_bytes[i]} for i, name in enumerate(_lib.GEMM_VARIANTS)}
        per["all"] = {k: sum(v[k] for v in per.values()) for k in ("launches", "flops", "ms", "bytes")}
        return per

    def profile_hbm_stats(self) -> dict:
        """The HBM-bound kernels timed since ``profile(True)``: launches, summed
        ms, algorithmic bytes and achieved GB/s per kind (include/tvr.h
        tvr_hbm_kind)."""
        st = _lib.CHbmStats()
        _lib.check(self._lib.tvr_profile_read_hbm(self._h, ctypes.byref(st)), "tvr_profile_read_hbm")
        return {name: {"launches": st.launches[i], "ms": st.ms[i], "bytes": st.bytes[i],
                       "gbps": st.bytes[i] / (st.ms[i] * 1e-3) / 1e9 if st.ms[i] > 0 else None}
                for i, name in enumerate(_lib.HBM_KINDS)}

    # ------------------------------------------------- TL-style conveniences
    def _as_ids(self, tokens) -> List[int]:
        if isinstance(tokens, str):
            tokens = self.to_tokens(tokens)
        if isinstance(tokens, torch.Tensor):
            if tokens.dim() == 2:
                if tokens.shape[0] != 1:
                    raise ValueError("batch size must be 1")
                tokens = tokens[0]
            return [int(x) for x in tokens.tolist()]
        return [int(x) for x in tokens]

    def forward(self, tokens, start_at_layer: Optional[int] = None, last_only: bool = False) -> torch.Tensor:
        """TransformerLens ``HookedTransformer.forward`` (scratch2.py:143,183,297;
        scratch.py:127,143,206,209) for batch 1: ``tokens`` (a string, ids [T]
        or [1, T]) -> logits [1, T, V] of every position; with
        ``start_at_layer=L``, ``tokens`` is the residual ``hook_resid_pre`` of
        block L ([1, T, d] or [T, d]) and the forward continues from there.
        ``last_only`` returns [1, 1, V] (the only row the reference reads)
        without the other rows' unembedding.  Up to n_ctx tokens."""
        dev, V = self.device, self.cfg.d_vocab
        if start_at_layer is None:
            ids = self._as_ids(tokens)
            if last_only:
                return self.forward_clean([ids], return_logits=True)["logits"].view(1, 1, -1)
            toks, lens = self._pack([ids])
            out = self._op("forward_logits", self._h.value, torch.from_numpy(toks), None, 0, torch.from_numpy(lens),
                           V, dev)
        else:
            resid = torch.as_tensor(tokens).to(dev, torch.float32)
            if resid.dim() == 3:
                if resid.shape[0] != 1:
                    raise ValueError("batch size must be 1")
                resid = resid[0]
            if resid.dim() != 2 or resid.shape[1] != self.cfg.d_model:
                raise ValueError("start_at_layer needs a residual of shape [1, T, d_model]")
            resid = resid.contiguous()
            lens = np.asarray([resid.shape[0]], dtype=np.int32)
            out = self._op("forward_logits", self._h.value, None, resid, int(start_at_layer), torch.from_numpy(lens),
                           V, dev)
        self._check_range("tvr_forward_logits")
        if last_only:
            out = out[-1:]
        return out.view(1, out.shape[0], V)

    __call__ = forward
