// torch_ops.cpp — the engine's entry points as torch.library operators
// (namespace ``tvr``), a thin layer over the C ABI of include/tvr.h
// (libtvr.so).  SURVEY.md §8(b): the façade calls ``torch.ops.tvr.*`` so the
// engine composes with torch's streams, allocator and graphs instead of
// taking raw pointers from Python.
//
//   tvr::forward_clean   tvr_forward_clean / _deferred   (scratch2.py:96,143,183)
//   tvr::patch_sweep     tvr_patch_sweep                 (scratch2.py:122-125,185-194)
//   tvr::patch_sweep_sets tvr_patch_sweep_sets           (several scratch2.py:188 hooks in one run_with_hooks)
//   tvr::patch_sweep_knockout tvr_patch_sweep_knockout   (hook_attn_scores[0, h, -1, keys] = -inf hooks in one run)
//   tvr::attention_knockout tvr_attention_knockout       (the knockout kernel alone, a test primitive)
//   tvr::project_heads   tvr_project_heads               (scratch2.py:97-98)
//   tvr::forward_logits  tvr_forward_logits              (scratch.py:143,206,209)
//   tvr::capture_resid   tvr_trace_capture_resid         (run_with_cache + hook_resid_pre[l][0, pos], summed)
//   tvr::capture_pattern tvr_trace_capture_pattern       (run_with_cache + cache["pattern", l][0, :, pos, :])
//   tvr::head_attribution tvr_head_attribution           (einsum of z, W_O and a direction per head)
//   tvr::logit_attribution tvr_trace_logit_attribution   (stack_head_results / accumulated_resid + logit_attrs)
//   tvr::logit_lens      tvr_trace_logit_lens            (ln_final + unembed of every layer's resid_pre row)
//   tvr::decode_rows     tvr_decode_rows                 (ln_final + unembed of any vectors)
//   tvr::head_directions tvr_head_directions             (dirs @ W_O[l]: a direction in the heads' z coordinates)
//   tvr::attention_source tvr_attention_source           (the source kernel alone, a test primitive)
//   tvr::source_attribution tvr_trace_source_attribution (pattern[q, j] * (v[j] @ W_O[h]) . dir per key j)
//
// Every op enqueues on torch's CURRENT stream of the output device and
// allocates its outputs through torch's caching allocator; host arrays
// (token ids, lengths, targets, site records) are CPU int32 tensors, the
// handles the int64 values of the tvr_model* / tvr_trace* the façade created.
// Status codes become exceptions with the engine's message: TVR_ERR_INVALID
// raises ValueError (the reference's shape errors, scratch2.py:172-175),
// everything else RuntimeError.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <string>
#include <tuple>
#include <vector>

#include "tvr.h"

namespace {

void check(int rc, const char* what) {
  if (rc == TVR_OK) return;
  const std::string msg = std::string(what) + ": " + tvr_last_error();
  TORCH_CHECK_VALUE(rc != TVR_ERR_INVALID, msg);
  TORCH_CHECK(false, msg, " (status ", rc, ")");
}

tvr_model* as_model(int64_t h) {
  TORCH_CHECK_VALUE(h != 0, "tvr: null model handle");
  return reinterpret_cast<tvr_model*>(static_cast<intptr_t>(h));
}

// torch's ROCm build presents HIP devices as DeviceType::CUDA: its guard and
// current-stream accessors are the "masquerading" ones
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

void* cur_stream(const c10::Device& dev) { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream(); }

void need_gpu(const c10::Device& dev) {
  TORCH_CHECK(dev.is_cuda(), "the HIP engine needs a GPU device (no CPU fallback): got device ", dev);
}

const int32_t* host_i32(const at::Tensor& t, const char* name) {
  TORCH_CHECK_VALUE(t.device().is_cpu() && t.scalar_type() == at::kInt && t.is_contiguous(), "tvr: ", name,
                    " must be a contiguous CPU int32 tensor");
  return t.data_ptr<int32_t>();
}

const int32_t* opt_host_i32(const std::optional<at::Tensor>& t, const char* name) {
  return t.has_value() ? host_i32(*t, name) : nullptr;
}

const float* in_f32(const std::optional<at::Tensor>& t, const c10::Device& dev, const char* name) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK_VALUE(t->device() == dev && t->scalar_type() == at::kFloat && t->is_contiguous(), "tvr: ", name,
                    " must be a contiguous fp32 tensor on ", dev);
  return t->data_ptr<float>();
}

at::TensorOptions f32(const c10::Device& dev) { return at::TensorOptions().dtype(at::kFloat).device(dev); }

// (prob [n], topk [n, k] int32, logits [n, V], zsum [L, d]); outputs not
// requested are empty tensors.  defer: tvr_forward_clean_deferred (the next
// patch_sweep on the trace writes prob / topk).
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> forward_clean(
    int64_t model, int64_t trace, const at::Tensor& tokens, const at::Tensor& seq_lens,
    const std::optional<at::Tensor>& targets, int64_t topk, bool want_logits, bool capture, bool defer,
    int64_t n_layers, int64_t d_model, int64_t d_vocab, c10::Device device) {
  const int64_t n = seq_lens.numel();
  TORCH_CHECK_VALUE(n > 0, "tvr: no prompts");
  need_gpu(device);
  DeviceGuard guard(device);
  const int32_t* tg = opt_host_i32(targets, "targets");
  TORCH_CHECK_VALUE(!targets.has_value() || targets->numel() == n, "targets must have one entry per prompt");
  auto prob = tg ? at::empty({n}, f32(device)) : at::empty({0}, f32(device));
  auto top = at::empty({topk ? n : 0, topk}, at::TensorOptions().dtype(at::kInt).device(device));
  auto logits = want_logits ? at::empty({n, d_vocab}, f32(device)) : at::empty({0}, f32(device));
  auto zsum = capture ? at::zeros({n_layers, d_model}, f32(device)) : at::empty({0}, f32(device));
  auto* tr = reinterpret_cast<tvr_trace*>(static_cast<intptr_t>(trace));
  void* st = cur_stream(device);
  if (defer) {
    TORCH_CHECK_VALUE(tr && !want_logits && !capture, "defer needs a trace and no logits / capture");
    check(tvr_forward_clean_deferred(as_model(model), tr, host_i32(tokens, "tokens"), host_i32(seq_lens, "seq_lens"),
                                     (int32_t)n, tg, tg ? prob.data_ptr<float>() : nullptr,
                                     topk ? top.data_ptr<int32_t>() : nullptr, (int32_t)topk, st),
          "tvr_forward_clean_deferred");
  } else {
    check(tvr_forward_clean(as_model(model), tr, host_i32(tokens, "tokens"), host_i32(seq_lens, "seq_lens"),
                            (int32_t)n, tg, tg ? prob.data_ptr<float>() : nullptr,
                            topk ? top.data_ptr<int32_t>() : nullptr, (int32_t)topk,
                            want_logits ? logits.data_ptr<float>() : nullptr,
                            capture ? zsum.data_ptr<float>() : nullptr, st),
          "tvr_forward_clean");
  }
  return {prob, top, logits, zsum};
}

// sites: CPU int32 [n_sites, 9] in tvr_site field order
std::tuple<at::Tensor, at::Tensor, at::Tensor> patch_sweep(int64_t model, int64_t trace, const at::Tensor& sites,
                                                           const std::optional<at::Tensor>& vectors, int64_t topk,
                                                           bool want_prob, bool want_logits, int64_t d_vocab,
                                                           c10::Device device) {
  static_assert(sizeof(tvr_site) == 9 * sizeof(int32_t), "tvr_site is 9 int32 fields");
  TORCH_CHECK_VALUE(sites.dim() == 2 && sites.size(1) == 9, "tvr: sites must be [n_sites, 9] int32");
  const int64_t n = sites.size(0);
  TORCH_CHECK_VALUE(n > 0, "tvr: no patch sites");
  TORCH_CHECK_VALUE(trace != 0, "tvr: patch_sweep needs a trace");
  need_gpu(device);
  DeviceGuard guard(device);
  const float* vec = in_f32(vectors, device, "vectors");
  const int32_t nvec = vectors.has_value() ? (int32_t)(vectors->numel() / std::max<int64_t>(vectors->size(-1), 1)) : 0;
  auto prob = want_prob ? at::empty({n}, f32(device)) : at::empty({0}, f32(device));
  auto top = at::empty({topk ? n : 0, topk}, at::TensorOptions().dtype(at::kInt).device(device));
  auto logits = want_logits ? at::empty({n, d_vocab}, f32(device)) : at::empty({0}, f32(device));
  check(tvr_patch_sweep(as_model(model), reinterpret_cast<tvr_trace*>(static_cast<intptr_t>(trace)),
                        reinterpret_cast<const tvr_site*>(host_i32(sites, "sites")), (int32_t)n, vec, nvec,
                        want_prob ? prob.data_ptr<float>() : nullptr, topk ? top.data_ptr<int32_t>() : nullptr,
                        (int32_t)topk, want_logits ? logits.data_ptr<float>() : nullptr, cur_stream(device)),
        "tvr_patch_sweep");
  return {prob, top, logits};
}

// patch_sweep with head-set sites (tvr_patch_sweep_sets).  set_off: CPU int32 [n_sites + 1]; patches: CPU
// int32 [n_patches, 3] in tvr_head_patch field order (layer, head, vec).  vectors needs only float
// alignment (an offset view is fine), so it is not required to be a fresh allocation — but contiguous.
std::tuple<at::Tensor, at::Tensor, at::Tensor> patch_sweep_sets(int64_t model, int64_t trace, const at::Tensor& sites,
                                                                const at::Tensor& set_off, const at::Tensor& patches,
                                                                const std::optional<at::Tensor>& vectors,
                                                                int64_t topk, bool want_prob, bool want_logits,
                                                                int64_t d_vocab, c10::Device device) {
  static_assert(sizeof(tvr_site) == 9 * sizeof(int32_t), "tvr_site is 9 int32 fields");
  static_assert(sizeof(tvr_head_patch) == 3 * sizeof(int32_t), "tvr_head_patch is 3 int32 fields");
  TORCH_CHECK_VALUE(sites.dim() == 2 && sites.size(1) == 9, "tvr: sites must be [n_sites, 9] int32");
  const int64_t n = sites.size(0);
  TORCH_CHECK_VALUE(n > 0, "tvr: no patch sites");
  TORCH_CHECK_VALUE(trace != 0, "tvr: patch_sweep_sets needs a trace");
  TORCH_CHECK_VALUE(set_off.dim() == 1 && set_off.numel() == n + 1, "tvr: set_off must be [n_sites + 1] int32");
  TORCH_CHECK_VALUE(patches.dim() == 2 && patches.size(1) == 3, "tvr: patches must be [n_patches, 3] int32");
  const int32_t* off = host_i32(set_off, "set_off");
  const int32_t* pat = host_i32(patches, "patches");
  // the C ABI trusts set_off[n_sites] as the length of patches: check it against the tensor here
  TORCH_CHECK_VALUE(off[0] >= 0 && off[n] <= patches.size(0), "tvr: set_off runs past patches (", off[n], " > ",
                    patches.size(0), ") or starts below 0");
  need_gpu(device);
  DeviceGuard guard(device);
  const float* vec = in_f32(vectors, device, "vectors");
  const int32_t nvec = vectors.has_value() ? (int32_t)(vectors->numel() / std::max<int64_t>(vectors->size(-1), 1)) : 0;
  auto prob = want_prob ? at::empty({n}, f32(device)) : at::empty({0}, f32(device));
  auto top = at::empty({topk ? n : 0, topk}, at::TensorOptions().dtype(at::kInt).device(device));
  auto logits = want_logits ? at::empty({n, d_vocab}, f32(device)) : at::empty({0}, f32(device));
  check(tvr_patch_sweep_sets(as_model(model), reinterpret_cast<tvr_trace*>(static_cast<intptr_t>(trace)),
                             reinterpret_cast<const tvr_site*>(host_i32(sites, "sites")), (int32_t)n, off,
                             reinterpret_cast<const tvr_head_patch*>(pat), vec, nvec,
                             want_prob ? prob.data_ptr<float>() : nullptr, topk ? top.data_ptr<int32_t>() : nullptr,
                             (int32_t)topk, want_logits ? logits.data_ptr<float>() : nullptr, cur_stream(device)),
        "tvr_patch_sweep_sets");
  return {prob, top, logits};
}

// patch_sweep_sets with attention-knockout sites (tvr_patch_sweep_knockout).  key_off: CPU int32 [n_sites + 1];
// keys: CPU int32 [n_keys], the blocked key positions of the kind-7 sites.
std::tuple<at::Tensor, at::Tensor, at::Tensor> patch_sweep_knockout(
    int64_t model, int64_t trace, const at::Tensor& sites, const at::Tensor& set_off, const at::Tensor& patches,
    const at::Tensor& key_off, const at::Tensor& keys, const std::optional<at::Tensor>& vectors, int64_t topk,
    bool want_prob, bool want_logits, int64_t d_vocab, c10::Device device) {
  static_assert(sizeof(tvr_site) == 9 * sizeof(int32_t), "tvr_site is 9 int32 fields");
  static_assert(sizeof(tvr_head_patch) == 3 * sizeof(int32_t), "tvr_head_patch is 3 int32 fields");
  TORCH_CHECK_VALUE(sites.dim() == 2 && sites.size(1) == 9, "tvr: sites must be [n_sites, 9] int32");
  const int64_t n = sites.size(0);
  TORCH_CHECK_VALUE(n > 0, "tvr: no patch sites");
  TORCH_CHECK_VALUE(trace != 0, "tvr: patch_sweep_knockout needs a trace");
  TORCH_CHECK_VALUE(set_off.dim() == 1 && set_off.numel() == n + 1, "tvr: set_off must be [n_sites + 1] int32");
  TORCH_CHECK_VALUE(key_off.dim() == 1 && key_off.numel() == n + 1, "tvr: key_off must be [n_sites + 1] int32");
  TORCH_CHECK_VALUE(patches.dim() == 2 && patches.size(1) == 3, "tvr: patches must be [n_patches, 3] int32");
  TORCH_CHECK_VALUE(keys.dim() == 1, "tvr: keys must be [n_keys] int32");
  const int32_t* off = host_i32(set_off, "set_off");
  const int32_t* pat = host_i32(patches, "patches");
  const int32_t* koff = host_i32(key_off, "key_off");
  const int32_t* kp = host_i32(keys, "keys");
  // the C ABI trusts the last offsets as the lengths of patches / keys: check them against the tensors here
  TORCH_CHECK_VALUE(off[0] >= 0 && off[n] <= patches.size(0), "tvr: set_off runs past patches (", off[n], " > ",
                    patches.size(0), ") or starts below 0");
  TORCH_CHECK_VALUE(koff[0] >= 0 && koff[n] <= keys.numel(), "tvr: key_off runs past keys (", koff[n], " > ",
                    keys.numel(), ") or starts below 0");
  need_gpu(device);
  DeviceGuard guard(device);
  const float* vec = in_f32(vectors, device, "vectors");
  const int32_t nvec = vectors.has_value() ? (int32_t)(vectors->numel() / std::max<int64_t>(vectors->size(-1), 1)) : 0;
  auto prob = want_prob ? at::empty({n}, f32(device)) : at::empty({0}, f32(device));
  auto top = at::empty({topk ? n : 0, topk}, at::TensorOptions().dtype(at::kInt).device(device));
  auto logits = want_logits ? at::empty({n, d_vocab}, f32(device)) : at::empty({0}, f32(device));
  check(tvr_patch_sweep_knockout(as_model(model), reinterpret_cast<tvr_trace*>(static_cast<intptr_t>(trace)),
                                 reinterpret_cast<const tvr_site*>(host_i32(sites, "sites")), (int32_t)n, off,
                                 reinterpret_cast<const tvr_head_patch*>(pat), koff, kp, vec, nvec,
                                 want_prob ? prob.data_ptr<float>() : nullptr,
                                 topk ? top.data_ptr<int32_t>() : nullptr, (int32_t)topk,
                                 want_logits ? logits.data_ptr<float>() : nullptr, cur_stream(device)),
        "tvr_patch_sweep_knockout");
  return {prob, top, logits};
}

// One knockout launch on a caller's buffers (tvr_attention_knockout).  qkv [rows, 3 d] and cache [cache_rows, 3 d]
// (or None): contiguous fp32 device tensors; seqs: CPU int32 [n_seq, 6] in tvr_attn_seq field order; items: CPU
// int64 [n_items, 4] rows (seq, head mask, first_key, n_keys); keys: CPU int32 [n_keys]; z: the activation
// buffer, written in place in format fmt.
void attention_knockout(int64_t model, int64_t fmt, const at::Tensor& qkv, const std::optional<at::Tensor>& cache,
                        const at::Tensor& seqs, const at::Tensor& items, const at::Tensor& keys, at::Tensor& z,
                        const std::optional<at::Tensor>& cos_t, const std::optional<at::Tensor>& sin_t) {
  static_assert(sizeof(tvr_attn_seq) == 6 * sizeof(int32_t), "tvr_attn_seq is 6 int32 fields");
  const c10::Device dev = z.device();
  need_gpu(dev);
  TORCH_CHECK_VALUE(qkv.dim() == 2 && z.is_contiguous(), "tvr: qkv must be [rows, 3 d] and z contiguous");
  TORCH_CHECK_VALUE(seqs.dim() == 2 && seqs.size(1) == 6, "tvr: seqs must be [n_seq, 6] int32");
  TORCH_CHECK_VALUE(items.dim() == 2 && items.size(1) == 4 && items.device().is_cpu() &&
                        items.scalar_type() == at::kLong && items.is_contiguous(),
                    "tvr: items must be a contiguous CPU int64 tensor [n_items, 4]");
  TORCH_CHECK_VALUE(keys.dim() == 1, "tvr: keys must be [n_keys] int32");
  const int32_t* sq = host_i32(seqs, "seqs");
  const int32_t* kp = host_i32(keys, "keys");
  std::vector<tvr_knockout_item> its((size_t)items.size(0));
  const int64_t* ip = items.data_ptr<int64_t>();
  for (size_t i = 0; i < its.size(); ++i) {
    its[i].seq = (int32_t)ip[4 * i];
    its[i].heads = (uint64_t)ip[4 * i + 1];
    its[i].first_key = (int32_t)ip[4 * i + 2];
    its[i].n_keys = (int32_t)ip[4 * i + 3];
  }
  DeviceGuard guard(dev);
  const float* q = in_f32(qkv, dev, "qkv");
  const float* cp = in_f32(cache, dev, "cache");
  check(tvr_attention_knockout(as_model(model), (int32_t)fmt, q, cp, reinterpret_cast<const tvr_attn_seq*>(sq),
                               (int32_t)seqs.size(0), (int32_t)qkv.size(0),
                               cache.has_value() ? (int32_t)cache->size(0) : 0, its.data(), (int32_t)its.size(), kp,
                               (int32_t)keys.numel(), z.data_ptr(), in_f32(cos_t, dev, "cos_t"),
                               in_f32(sin_t, dev, "sin_t"), cur_stream(dev)),
        "tvr_attention_knockout");
}

// zsum [L, d] -> [L, H, d]
at::Tensor project_heads(int64_t model, const at::Tensor& zsum, int64_t n_heads) {
  TORCH_CHECK_VALUE(zsum.dim() == 2, "tvr: zsum must be [n_layers, d_model]");
  const c10::Device dev = zsum.device();
  need_gpu(dev);
  DeviceGuard guard(dev);
  const float* z = in_f32(zsum, dev, "zsum");
  auto out = at::empty({zsum.size(0), n_heads, zsum.size(1)}, f32(dev));
  check(tvr_project_heads(as_model(model), z, out.data_ptr<float>(), cur_stream(dev)), "tvr_project_heads");
  return out;
}

// logits of every position [sum(seq_lens), V]; exactly one of tokens (host ids)
// and resid (device [sum(seq_lens), d] entering block start_layer)
at::Tensor forward_logits(int64_t model, const std::optional<at::Tensor>& tokens,
                          const std::optional<at::Tensor>& resid, int64_t start_layer, const at::Tensor& seq_lens,
                          int64_t d_vocab, c10::Device device) {
  need_gpu(device);
  DeviceGuard guard(device);
  const int32_t* lens = host_i32(seq_lens, "seq_lens");
  int64_t rows = 0;
  for (int64_t i = 0; i < seq_lens.numel(); ++i) rows += lens[i];
  auto out = at::empty({rows, d_vocab}, f32(device));
  check(tvr_forward_logits(as_model(model), opt_host_i32(tokens, "tokens"), in_f32(resid, device, "resid"),
                           (int32_t)start_layer, lens, (int32_t)seq_lens.numel(), out.data_ptr<float>(),
                           cur_stream(device)),
        "tvr_forward_logits");
  return out;
}

// out [n_groups, L + 1, d] += the grouped sums of hook_resid_pre rows (tvr_trace_capture_resid).  pos / groups:
// CPU int32 [n_seq] or None; out: a contiguous fp32 device tensor (an offset view is fine: float alignment
// suffices), whose size the façade checks against the trace's model.  Returns out.
at::Tensor& capture_resid(int64_t trace, const std::optional<at::Tensor>& pos, const std::optional<at::Tensor>& groups,
                          int64_t n_groups, int64_t n_seq, at::Tensor& out) {
  TORCH_CHECK_VALUE(trace != 0, "tvr: capture_resid needs a trace");
  TORCH_CHECK_VALUE(n_groups > 0, "tvr: n_groups must be positive");
  TORCH_CHECK_VALUE(!pos.has_value() || pos->numel() == n_seq, "tvr: pos must have one entry per traced sequence");
  TORCH_CHECK_VALUE(!groups.has_value() || groups->numel() == n_seq,
                    "tvr: groups must have one entry per traced sequence");
  const c10::Device dev = out.device();
  need_gpu(dev);
  TORCH_CHECK_VALUE(out.scalar_type() == at::kFloat && out.is_contiguous() && out.dim() == 3 && out.size(0) == n_groups,
                    "tvr: out must be a contiguous fp32 tensor [n_groups, n_layers + 1, d_model]");
  DeviceGuard guard(dev);
  check(tvr_trace_capture_resid(reinterpret_cast<tvr_trace*>(static_cast<intptr_t>(trace)), opt_host_i32(pos, "pos"),
                                opt_host_i32(groups, "groups"), (int32_t)n_groups, out.data_ptr<float>(),
                                cur_stream(dev)),
        "tvr_trace_capture_resid");
  return out;
}

// One query's attention pattern per traced sequence, every layer and head (tvr_trace_capture_pattern).  pos: CPU
// int32 [n_seq] or None (last position); cls: CPU int32 [traced tokens] or None; out_pattern [n_seq, L, H, ld] and
// out_mass [n_seq, L, H, n_classes]: contiguous fp32 device tensors (offset views are fine: float alignment
// suffices), at least one of them.  The façade sizes them from the trace's model.
void capture_pattern(int64_t trace, const std::optional<at::Tensor>& pos, const std::optional<at::Tensor>& cls,
                     int64_t n_classes, int64_t n_seq, int64_t n_layers, int64_t n_heads,
                     const std::optional<at::Tensor>& out_pattern, const std::optional<at::Tensor>& out_mass) {
  TORCH_CHECK_VALUE(trace != 0, "tvr: capture_pattern needs a trace");
  TORCH_CHECK_VALUE(out_pattern.has_value() || out_mass.has_value(), "tvr: capture_pattern needs out_pattern or out_mass");
  TORCH_CHECK_VALUE(!pos.has_value() || pos->numel() == n_seq, "tvr: pos must have one entry per traced sequence");
  TORCH_CHECK_VALUE(!out_mass.has_value() || cls.has_value(), "tvr: out_mass needs cls");
  TORCH_CHECK_VALUE(!cls.has_value() || n_classes > 0, "tvr: n_classes must be positive");
  const c10::Device dev = out_pattern.has_value() ? out_pattern->device() : out_mass->device();
  need_gpu(dev);
  auto shaped = [&](const at::Tensor& t, int64_t last) {
    return t.device() == dev && t.scalar_type() == at::kFloat && t.is_contiguous() && t.dim() == 4 &&
           t.size(0) == n_seq && t.size(1) == n_layers && t.size(2) == n_heads && (last < 0 || t.size(3) == last);
  };
  TORCH_CHECK_VALUE(!out_pattern.has_value() || shaped(*out_pattern, -1),
                    "tvr: out_pattern must be a contiguous fp32 tensor [n_seq, n_layers, n_heads, ld]");
  TORCH_CHECK_VALUE(!out_mass.has_value() || shaped(*out_mass, n_classes),
                    "tvr: out_mass must be a contiguous fp32 tensor [n_seq, n_layers, n_heads, n_classes]");
  auto* tr = reinterpret_cast<tvr_trace*>(static_cast<intptr_t>(trace));
  // the C ABI trusts cls to hold one entry per traced token: check it against the tensor here
  TORCH_CHECK_VALUE(!cls.has_value() || cls->numel() == tvr_trace_num_tokens(tr),
                    "tvr: cls must have one entry per traced token");
  DeviceGuard guard(dev);
  check(tvr_trace_capture_pattern(tr, opt_host_i32(pos, "pos"), opt_host_i32(cls, "cls"), (int32_t)n_classes,
                                  out_pattern.has_value() ? out_pattern->data_ptr<float>() : nullptr,
                                  out_pattern.has_value() ? (int32_t)out_pattern->size(3) : 0,
                                  out_mass.has_value() ? out_mass->data_ptr<float>() : nullptr, cur_stream(dev)),
        "tvr_trace_capture_pattern");
}

bool dev_tensor(const at::Tensor& t, const c10::Device& dev, at::ScalarType ty) {
  return t.device() == dev && t.scalar_type() == ty && t.is_contiguous();
}

// out [n, H] = per-head attribution of z [n, d] along dirs [n, d] at one layer (tvr_head_attribution).  z and
// dirs: contiguous fp32 device tensors whose storage is 16-byte aligned (the engine refuses others); out: a
// contiguous fp32 device tensor, an offset view is fine.  d_model / n_heads: the model's, which the widths must equal.
void head_attribution(int64_t model, int64_t layer, const at::Tensor& z, const at::Tensor& dirs, int64_t d_model,
                      int64_t n_heads, at::Tensor& out) {
  const c10::Device dev = out.device();
  need_gpu(dev);
  TORCH_CHECK_VALUE(z.dim() == 2 && z.size(0) > 0 && z.size(1) == d_model && dev_tensor(z, dev, at::kFloat) &&
                        dirs.sizes() == z.sizes() && dev_tensor(dirs, dev, at::kFloat),
                    "tvr: z and dirs must be contiguous fp32 tensors [n, d_model] on the output's device");
  TORCH_CHECK_VALUE(dev_tensor(out, dev, at::kFloat) && out.dim() == 2 && out.size(0) == z.size(0) &&
                        out.size(1) == n_heads,
                    "tvr: out must be a contiguous fp32 tensor [n, n_heads]");
  DeviceGuard guard(dev);
  check(tvr_head_attribution(as_model(model), (int32_t)layer, z.data_ptr<float>(), dirs.data_ptr<float>(),
                             (int32_t)z.size(0), out.data_ptr<float>(), cur_stream(dev)),
        "tvr_head_attribution");
}

// Direct logit attribution of a trace (tvr_trace_logit_attribution).  pos / contrast: CPU int32 [n_seq] or None;
// target: CPU int32 [n_seq]; out_head [n_seq, L, H] and out_resid [n_seq, L + 1]: contiguous fp32 device tensors,
// at least one of them.
void logit_attribution(int64_t trace, const std::optional<at::Tensor>& pos, const at::Tensor& target,
                       const std::optional<at::Tensor>& contrast, int64_t n_seq, int64_t n_layers, int64_t n_heads,
                       const std::optional<at::Tensor>& out_head, const std::optional<at::Tensor>& out_resid) {
  TORCH_CHECK_VALUE(trace != 0, "tvr: logit_attribution needs a trace");
  TORCH_CHECK_VALUE(out_head.has_value() || out_resid.has_value(), "tvr: logit_attribution needs out_head or out_resid");
  TORCH_CHECK_VALUE(!pos.has_value() || pos->numel() == n_seq, "tvr: pos must have one entry per traced sequence");
  TORCH_CHECK_VALUE(target.numel() == n_seq, "tvr: target must have one entry per traced sequence");
  TORCH_CHECK_VALUE(!contrast.has_value() || contrast->numel() == n_seq,
                    "tvr: contrast must have one entry per traced sequence");
  const c10::Device dev = out_head.has_value() ? out_head->device() : out_resid->device();
  need_gpu(dev);
  TORCH_CHECK_VALUE(!out_head.has_value() || (dev_tensor(*out_head, dev, at::kFloat) && out_head->dim() == 3 &&
                                              out_head->size(0) == n_seq && out_head->size(1) == n_layers &&
                                              out_head->size(2) == n_heads),
                    "tvr: out_head must be a contiguous fp32 tensor [n_seq, n_layers, n_heads]");
  TORCH_CHECK_VALUE(!out_resid.has_value() || (dev_tensor(*out_resid, dev, at::kFloat) && out_resid->dim() == 2 &&
                                               out_resid->size(0) == n_seq && out_resid->size(1) == n_layers + 1),
                    "tvr: out_resid must be a contiguous fp32 tensor [n_seq, n_layers + 1]");
  DeviceGuard guard(dev);
  check(tvr_trace_logit_attribution(reinterpret_cast<tvr_trace*>(static_cast<intptr_t>(trace)),
                                    opt_host_i32(pos, "pos"), host_i32(target, "target"),
                                    opt_host_i32(contrast, "contrast"),
                                    out_head.has_value() ? out_head->data_ptr<float>() : nullptr,
                                    out_resid.has_value() ? out_resid->data_ptr<float>() : nullptr, cur_stream(dev)),
        "tvr_trace_logit_attribution");
}

// out_g [n, d_model] = dirs [n, d_model] pulled back through W_O of one layer (tvr_head_directions).  dirs and
// out_g: contiguous fp32 device tensors whose storage is 16-byte aligned (the engine refuses others).
void head_directions(int64_t model, int64_t layer, const at::Tensor& dirs, int64_t d_model, at::Tensor& out_g) {
  const c10::Device dev = out_g.device();
  need_gpu(dev);
  TORCH_CHECK_VALUE(dirs.dim() == 2 && dirs.size(0) > 0 && dirs.size(1) == d_model && dev_tensor(dirs, dev, at::kFloat),
                    "tvr: dirs must be a contiguous fp32 tensor [n, d_model] on the output's device");
  TORCH_CHECK_VALUE(dev_tensor(out_g, dev, at::kFloat) && out_g.sizes() == dirs.sizes(),
                    "tvr: out_g must be a contiguous fp32 tensor [n, d_model]");
  DeviceGuard guard(dev);
  check(tvr_head_directions(as_model(model), (int32_t)layer, dirs.data_ptr<float>(), (int32_t)dirs.size(0),
                            out_g.data_ptr<float>(), cur_stream(dev)),
        "tvr_head_directions");
}

// The source kernel on a caller's one-layer buffer (tvr_attention_source).  qkv [rows, 3 d_model] and g
// [n_seq, d_model]: contiguous fp32 device tensors, 16-byte aligned; row0 / qpos: CPU int32 [n_seq]; cls: CPU
// int32 [rows] or None; out_src [n_seq, n_heads, ld] and out_cls [n_seq, n_heads, n_classes]: contiguous fp32
// device tensors (offset views are fine), at least one of them; cos_t / sin_t: device tables or None (the model's).
void attention_source(int64_t model, const at::Tensor& qkv, const at::Tensor& row0, const at::Tensor& qpos,
                      const at::Tensor& g, const std::optional<at::Tensor>& cls, int64_t n_classes, int64_t d_model,
                      int64_t n_heads, const std::optional<at::Tensor>& out_src, const std::optional<at::Tensor>& out_cls,
                      const std::optional<at::Tensor>& cos_t, const std::optional<at::Tensor>& sin_t) {
  TORCH_CHECK_VALUE(out_src.has_value() || out_cls.has_value(), "tvr: attention_source needs out_src or out_cls");
  TORCH_CHECK_VALUE(!out_cls.has_value() || cls.has_value(), "tvr: out_cls needs cls");
  TORCH_CHECK_VALUE(!cls.has_value() || n_classes > 0, "tvr: n_classes must be positive");
  const int64_t n_seq = row0.numel();
  TORCH_CHECK_VALUE(n_seq > 0 && qpos.numel() == n_seq, "tvr: row0 and qpos must have one entry per sequence");
  const c10::Device dev = out_src.has_value() ? out_src->device() : out_cls->device();
  need_gpu(dev);
  TORCH_CHECK_VALUE(qkv.dim() == 2 && qkv.size(0) > 0 && qkv.size(1) == 3 * d_model && dev_tensor(qkv, dev, at::kFloat),
                    "tvr: qkv must be a contiguous fp32 tensor [rows, 3 d_model] on the outputs' device");
  TORCH_CHECK_VALUE(g.dim() == 2 && g.size(0) == n_seq && g.size(1) == d_model && dev_tensor(g, dev, at::kFloat),
                    "tvr: g must be a contiguous fp32 tensor [n_seq, d_model] on the outputs' device");
  TORCH_CHECK_VALUE(!cls.has_value() || cls->numel() == qkv.size(0), "tvr: cls must have one entry per row of qkv");
  auto shaped = [&](const at::Tensor& t, int64_t last) {
    return dev_tensor(t, dev, at::kFloat) && t.dim() == 3 && t.size(0) == n_seq && t.size(1) == n_heads &&
           (last < 0 || t.size(2) == last);
  };
  TORCH_CHECK_VALUE(!out_src.has_value() || shaped(*out_src, -1),
                    "tvr: out_src must be a contiguous fp32 tensor [n_seq, n_heads, ld]");
  TORCH_CHECK_VALUE(!out_cls.has_value() || shaped(*out_cls, n_classes),
                    "tvr: out_cls must be a contiguous fp32 tensor [n_seq, n_heads, n_classes]");
  DeviceGuard guard(dev);
  check(tvr_attention_source(as_model(model), qkv.data_ptr<float>(), (int32_t)qkv.size(0), host_i32(row0, "row0"),
                             host_i32(qpos, "qpos"), (int32_t)n_seq, g.data_ptr<float>(), opt_host_i32(cls, "cls"),
                             (int32_t)n_classes, out_src.has_value() ? out_src->data_ptr<float>() : nullptr,
                             out_src.has_value() ? (int32_t)out_src->size(2) : 0,
                             out_cls.has_value() ? out_cls->data_ptr<float>() : nullptr, in_f32(cos_t, dev, "cos_t"),
                             in_f32(sin_t, dev, "sin_t"), cur_stream(dev)),
        "tvr_attention_source");
}

// Per-source-token logit attribution of a trace (tvr_trace_source_attribution).  pos / contrast: CPU int32 [n_seq]
// or None; target: CPU int32 [n_seq]; cls: CPU int32 [traced tokens] or None; out_src [n_seq, L, H, ld] and
// out_cls [n_seq, L, H, n_classes]: contiguous fp32 device tensors (offset views are fine), at least one of them.
void source_attribution(int64_t trace, const std::optional<at::Tensor>& pos, const at::Tensor& target,
                        const std::optional<at::Tensor>& contrast, const std::optional<at::Tensor>& cls,
                        int64_t n_classes, int64_t n_seq, int64_t n_layers, int64_t n_heads,
                        const std::optional<at::Tensor>& out_src, const std::optional<at::Tensor>& out_cls) {
  TORCH_CHECK_VALUE(trace != 0, "tvr: source_attribution needs a trace");
  TORCH_CHECK_VALUE(out_src.has_value() || out_cls.has_value(), "tvr: source_attribution needs out_src or out_cls");
  TORCH_CHECK_VALUE(!pos.has_value() || pos->numel() == n_seq, "tvr: pos must have one entry per traced sequence");
  TORCH_CHECK_VALUE(target.numel() == n_seq, "tvr: target must have one entry per traced sequence");
  TORCH_CHECK_VALUE(!contrast.has_value() || contrast->numel() == n_seq,
                    "tvr: contrast must have one entry per traced sequence");
  TORCH_CHECK_VALUE(!out_cls.has_value() || cls.has_value(), "tvr: out_cls needs cls");
  TORCH_CHECK_VALUE(!cls.has_value() || n_classes > 0, "tvr: n_classes must be positive");
  const c10::Device dev = out_src.has_value() ? out_src->device() : out_cls->device();
  need_gpu(dev);
  auto shaped = [&](const at::Tensor& t, int64_t last) {
    return dev_tensor(t, dev, at::kFloat) && t.dim() == 4 && t.size(0) == n_seq && t.size(1) == n_layers &&
           t.size(2) == n_heads && (last < 0 || t.size(3) == last);
  };
  TORCH_CHECK_VALUE(!out_src.has_value() || shaped(*out_src, -1),
                    "tvr: out_src must be a contiguous fp32 tensor [n_seq, n_layers, n_heads, ld]");
  TORCH_CHECK_VALUE(!out_cls.has_value() || shaped(*out_cls, n_classes),
                    "tvr: out_cls must be a contiguous fp32 tensor [n_seq, n_layers, n_heads, n_classes]");
  auto* tr = reinterpret_cast<tvr_trace*>(static_cast<intptr_t>(trace));
  // the C ABI trusts cls to hold one entry per traced token: check it against the tensor here
  TORCH_CHECK_VALUE(!cls.has_value() || cls->numel() == tvr_trace_num_tokens(tr),
                    "tvr: cls must have one entry per traced token");
  DeviceGuard guard(dev);
  check(tvr_trace_source_attribution(tr, opt_host_i32(pos, "pos"), host_i32(target, "target"),
                                     opt_host_i32(contrast, "contrast"), opt_host_i32(cls, "cls"), (int32_t)n_classes,
                                     out_src.has_value() ? out_src->data_ptr<float>() : nullptr,
                                     out_src.has_value() ? (int32_t)out_src->size(3) : 0,
                                     out_cls.has_value() ? out_cls->data_ptr<float>() : nullptr, cur_stream(dev)),
        "tvr_trace_source_attribution");
}

// The output pair of logit_lens / decode_rows: out_prob fp32 with `rows` elements, out_topk int32 [.., topk].
c10::Device decode_outputs(const std::optional<at::Tensor>& targets, int64_t n_targets, int64_t rows, int64_t topk,
                           const std::optional<at::Tensor>& out_prob, const std::optional<at::Tensor>& out_topk) {
  TORCH_CHECK_VALUE(out_prob.has_value() || out_topk.has_value(), "tvr: needs out_prob or out_topk");
  TORCH_CHECK_VALUE(!out_prob.has_value() || targets.has_value(), "tvr: out_prob needs targets");
  TORCH_CHECK_VALUE(!targets.has_value() || targets->numel() == n_targets, "tvr: targets must have one entry per row");
  const c10::Device dev = out_prob.has_value() ? out_prob->device() : out_topk->device();
  need_gpu(dev);
  TORCH_CHECK_VALUE(!out_prob.has_value() || (dev_tensor(*out_prob, dev, at::kFloat) && out_prob->numel() == rows),
                    "tvr: out_prob must be a contiguous fp32 tensor with one entry per decoded row");
  TORCH_CHECK_VALUE(!out_topk.has_value() || (topk > 0 && dev_tensor(*out_topk, dev, at::kInt) &&
                                              out_topk->numel() == rows * topk && out_topk->size(-1) == topk),
                    "tvr: out_topk must be a contiguous int32 tensor [rows, topk] with topk > 0");
  return dev;
}

// Logit lens of a trace (tvr_trace_logit_lens).  pos / targets: CPU int32 [n_seq] or None; out_prob
// [n_seq, L + 1] fp32 and out_topk [n_seq, L + 1, topk] int32: contiguous device tensors, at least one.
void logit_lens(int64_t trace, const std::optional<at::Tensor>& pos, const std::optional<at::Tensor>& targets,
                int64_t n_seq, int64_t n_layers, int64_t topk, const std::optional<at::Tensor>& out_prob,
                const std::optional<at::Tensor>& out_topk) {
  TORCH_CHECK_VALUE(trace != 0, "tvr: logit_lens needs a trace");
  TORCH_CHECK_VALUE(!pos.has_value() || pos->numel() == n_seq, "tvr: pos must have one entry per traced sequence");
  const c10::Device dev = decode_outputs(targets, n_seq, n_seq * (n_layers + 1), topk, out_prob, out_topk);
  DeviceGuard guard(dev);
  check(tvr_trace_logit_lens(reinterpret_cast<tvr_trace*>(static_cast<intptr_t>(trace)), opt_host_i32(pos, "pos"),
                             opt_host_i32(targets, "targets"),
                             out_prob.has_value() ? out_prob->data_ptr<float>() : nullptr,
                             out_topk.has_value() ? out_topk->data_ptr<int32_t>() : nullptr, (int32_t)topk,
                             cur_stream(dev)),
        "tvr_trace_logit_lens");
}

// Vocabulary decoding of rows [n, d] (tvr_decode_rows): a contiguous fp32 device tensor, 16-byte aligned.
void decode_rows(int64_t model, const at::Tensor& rows, const std::optional<at::Tensor>& targets, int64_t topk,
                 int64_t d_model, const std::optional<at::Tensor>& out_prob, const std::optional<at::Tensor>& out_topk) {
  TORCH_CHECK_VALUE(rows.dim() == 2 && rows.size(0) > 0 && rows.size(1) == d_model, "tvr: rows must be [n, d_model]");
  const c10::Device dev = decode_outputs(targets, rows.size(0), rows.size(0), topk, out_prob, out_topk);
  TORCH_CHECK_VALUE(dev_tensor(rows, dev, at::kFloat), "tvr: rows must be a contiguous fp32 tensor on the outputs' device");
  DeviceGuard guard(dev);
  check(tvr_decode_rows(as_model(model), rows.data_ptr<float>(), (int32_t)rows.size(0),
                        opt_host_i32(targets, "targets"), out_prob.has_value() ? out_prob->data_ptr<float>() : nullptr,
                        out_topk.has_value() ? out_topk->data_ptr<int32_t>() : nullptr, (int32_t)topk, cur_stream(dev)),
        "tvr_decode_rows");
}

}  // namespace

TORCH_LIBRARY(tvr, m) {
  m.def("forward_clean(int model, int trace, Tensor tokens, Tensor seq_lens, Tensor? targets, int topk, "
        "bool want_logits, bool capture, bool defer, int n_layers, int d_model, int d_vocab, Device device) "
        "-> (Tensor, Tensor, Tensor, Tensor)");
  m.def("patch_sweep(int model, int trace, Tensor sites, Tensor? vectors, int topk, bool want_prob, "
        "bool want_logits, int d_vocab, Device device) -> (Tensor, Tensor, Tensor)");
  m.def("patch_sweep_sets(int model, int trace, Tensor sites, Tensor set_off, Tensor patches, Tensor? vectors, "
        "int topk, bool want_prob, bool want_logits, int d_vocab, Device device) -> (Tensor, Tensor, Tensor)");
  m.def("patch_sweep_knockout(int model, int trace, Tensor sites, Tensor set_off, Tensor patches, Tensor key_off, "
        "Tensor keys, Tensor? vectors, int topk, bool want_prob, bool want_logits, int d_vocab, Device device) "
        "-> (Tensor, Tensor, Tensor)");
  m.def("attention_knockout(int model, int fmt, Tensor qkv, Tensor? cache, Tensor seqs, Tensor items, Tensor keys, "
        "Tensor(a!) z, Tensor? cos_t, Tensor? sin_t) -> ()");
  m.def("project_heads(int model, Tensor zsum, int n_heads) -> Tensor");
  m.def("forward_logits(int model, Tensor? tokens, Tensor? resid, int start_layer, Tensor seq_lens, int d_vocab, "
        "Device device) -> Tensor");
  m.def("capture_resid(int trace, Tensor? pos, Tensor? groups, int n_groups, int n_seq, Tensor(a!) out) -> Tensor(a!)");
  m.def("capture_pattern(int trace, Tensor? pos, Tensor? cls, int n_classes, int n_seq, int n_layers, int n_heads, "
        "Tensor(a!)? out_pattern, Tensor(b!)? out_mass) -> ()");
  m.def("head_attribution(int model, int layer, Tensor z, Tensor dirs, int d_model, int n_heads, Tensor(a!) out) -> ()");
  m.def("logit_attribution(int trace, Tensor? pos, Tensor target, Tensor? contrast, int n_seq, int n_layers, "
        "int n_heads, Tensor(a!)? out_head, Tensor(b!)? out_resid) -> ()");
  m.def("logit_lens(int trace, Tensor? pos, Tensor? targets, int n_seq, int n_layers, int topk, "
        "Tensor(a!)? out_prob, Tensor(b!)? out_topk) -> ()");
  m.def("decode_rows(int model, Tensor rows, Tensor? targets, int topk, int d_model, Tensor(a!)? out_prob, "
        "Tensor(b!)? out_topk) -> ()");
  m.def("head_directions(int model, int layer, Tensor dirs, int d_model, Tensor(a!) out_g) -> ()");
  m.def("attention_source(int model, Tensor qkv, Tensor row0, Tensor qpos, Tensor g, Tensor? cls, int n_classes, "
        "int d_model, int n_heads, Tensor(a!)? out_src, Tensor(b!)? out_cls, Tensor? cos_t, Tensor? sin_t) -> ()");
  m.def("source_attribution(int trace, Tensor? pos, Tensor target, Tensor? contrast, Tensor? cls, int n_classes, "
        "int n_seq, int n_layers, int n_heads, Tensor(a!)? out_src, Tensor(b!)? out_cls) -> ()");
}

// Mixed host / device tensor arguments: one implementation for every backend key.
TORCH_LIBRARY_IMPL(tvr, CompositeExplicitAutograd, m) {
  m.impl("forward_clean", &forward_clean);
  m.impl("patch_sweep", &patch_sweep);
  m.impl("patch_sweep_sets", &patch_sweep_sets);
  m.impl("patch_sweep_knockout", &patch_sweep_knockout);
  m.impl("attention_knockout", &attention_knockout);
  m.impl("project_heads", &project_heads);
  m.impl("forward_logits", &forward_logits);
  m.impl("capture_resid", &capture_resid);
  m.impl("capture_pattern", &capture_pattern);
  m.impl("head_attribution", &head_attribution);
  m.impl("logit_attribution", &logit_attribution);
  m.impl("logit_lens", &logit_lens);
  m.impl("decode_rows", &decode_rows);
  m.impl("head_directions", &head_directions);
  m.impl("attention_source", &attention_source);
  m.impl("source_attribution", &source_attribution);
}
