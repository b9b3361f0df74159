/*
 * tvr.h — C ABI of the MI355X-native task-vector / function-vector engine.
 *
 * The reference (IMMachinations/Task-Vector-Replication) drives every patched
 * forward through TransformerLens from Python loops:
 *   - extraction   scratch2.py:81-100   (run_with_cache + hook_result[0,-1])
 *   - layer sweeps scratch2.py:107-150  (run_with_hooks, hook_attn_out[0,-1] += v)
 *   - CIE sweep    scratch2.py:171-197  (run_with_hooks, hook_result[0,:,h] = mean)
 *   - FV eval      scratch2.py:292-314  (run_with_hooks + top-k)
 *   - resid patch  scratch.py:106-147   (cache surgery + forward(start_at_layer=L))
 * There is no native FFI in the reference: its Python façade binds these
 * entry points through ctypes.  Every entry point below
 * replaces one of those loops with ONE batched launch sequence whose batch
 * dimension enumerates patch sites.
 *
 * Conventions
 *   - Host arrays: token ids, sequence lengths, targets and site records.
 *   - Device arrays: weights, vectors and all outputs; owned by the caller
 *     (PyTorch) and preallocated.  Traces and the activation workspace are
 *     owned by the engine (allocated outside timed regions, reused).
 *   - `stream` is a hipStream_t passed as void*; everything is enqueued on it
 *     and nothing synchronises the host except tvr_*_create / destroy.
 *   - Every function returns TVR_OK (0) or a negative error code; no C++
 *     exception crosses the ABI.  tvr_last_error() explains the last failure
 *     on the calling thread.
 *   - Numerics: LayerNorm, attention, the residual stream, the injections and
 *     the softmax are fp32 (the reference's TransformerLens default dtype).
 *     The GEMMs run on the matrix-core path chosen by tvr_model_set_gemm:
 *     TVR_GEMM_F32 at tvr_model_create; the Python façade selects
 *     TVR_GEMM_X2F16, an fp32-accurate emulation (each fp32 operand as two
 *     fp16 planes, three fp16 MFMA products, fp32 accumulation), by default.
 */
#ifndef TVR_H_
#define TVR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TVR_ABI_VERSION 11

enum tvr_status {
  TVR_OK = 0,
  TVR_ERR_INVALID = -1,     /* bad argument / shape (reference: ValueError) */
  TVR_ERR_HIP = -2,         /* HIP runtime failure */
  TVR_ERR_NOMEM = -3,       /* device allocation failed */
  TVR_ERR_UNSUPPORTED = -4, /* shape outside what the kernels handle */
  TVR_ERR_RANGE = -5,       /* a GEMM input exceeded the TVR_GEMM_X2F16 range */
  TVR_ERR_INTERNAL = -6     /* an engine invariant failed (a bug: report it) */
};

/* Patch-site kinds: the declarative replacement for TransformerLens hooks. */
enum tvr_site_kind {
  /* No patch: re-evaluate the clean last-position distribution. */
  TVR_SITE_NONE = 0,
  /* blocks.{layer}.attn.hook_result[0,:,head,:] = vectors[vec] at every
   * position (scratch2.py:167-169, 187-189). */
  TVR_SITE_REPLACE_HEAD_ALLPOS = 1,
  /* blocks.{layer}.hook_attn_out[0,-1,:] += vectors[vec]
   * (scratch2.py:107-109). */
  TVR_SITE_ADD_ATTN_OUT_LASTPOS = 2,
  /* blocks.{layer}.hook_resid_pre of sequence `seq` with row `pos` replaced by
   * the same hook's row `src_pos` of sequence `src_seq`, then
   * forward(start_at_layer=layer) (scratch.py:140-143, 201-209). */
  TVR_SITE_SET_RESID_PRE_POS = 3,
  /* Joint head-set patches (tvr_patch_sweep_sets only): for EVERY member
   * (layer, head, vec) of the site's set,
   *   blocks.{layer}.attn.hook_result[0,:,head,:] = vectors[vec]   (ALLPOS:
   *   one scratch2.py:188 hook per member in one run_with_hooks call), or
   *   blocks.{layer}.attn.hook_result[0,-1,head,:] = vectors[vec]  (LASTPOS:
   *   the last-token intervention of the function-vector paper).
   * The site's own layer / head / vec fields are ignored. */
  TVR_SITE_REPLACE_HEADSET_ALLPOS = 4,
  TVR_SITE_REPLACE_HEADSET_LASTPOS = 5,
  /* blocks.{layer}.hook_resid_pre[0, pos, :] = vectors[vec], then
   * forward(start_at_layer=layer): a caller's vector written into the residual
   * stream (Hendel et al.'s task-vector patch: theta(layer) at the last position
   * of a zero-shot prompt).  Fields seq, layer, pos, vec, target.  Planned as
   * TVR_SITE_SET_RESID_PRE_POS: the site enters at `layer` and computes rows
   * [pos, T), so a last-position site is one row on the single-query attention.
   * `vectors` holds TransformerLens' (centred) residual values, e.g. rows of
   * tvr_trace_capture_resid or tvr_trace_read.  With exact-fp16 weights bound
   * (tvr_model_set_exact16) the clean rows carry one constant per row and the
   * vector is written as it is: the patched row's constant is then zero, which
   * every LayerNorm and the centred export tolerate (results equal the
   * processed-weight path's to fp32 rounding).  The entry kernel reads `vectors`
   * element-wise for this kind: float (4 B) alignment suffices.  Accepted by
   * tvr_patch_sweep and tvr_patch_sweep_sets (there it owns an empty patch
   * range); on a filled trace or a deferred clean forward, every GEMM path.
   * TVR_ERR_INVALID for layer, pos or vec out of range or null vectors.
   * (Backward-compatible addition: ABI 11.) */
  TVR_SITE_SET_RESID_PRE_VEC = 6,
  /* Attention knockout of the last token (tvr_patch_sweep_knockout only): for
   * every member (layer, head) of the site's set and every blocked key j of its
   * key list, blocks.{layer}.attn.hook_attn_scores[0, head, -1, j] = -inf in one
   * forward: hook_pattern[0, head, -1, :] is the softmax over the remaining keys
   * and 0 on the blocked ones, hook_z[0, -1, head] that pattern times V, and
   * everything downstream follows.  Other heads and other positions are
   * untouched.  Fields seq and target; layer / head / vec are ignored.
   * (Backward-compatible addition: ABI 11.) */
  TVR_SITE_ATTN_KNOCKOUT_LASTPOS = 7
};

typedef struct tvr_config {
  int32_t n_layers;
  int32_t d_model;
  int32_t n_heads;
  int32_t d_head;
  int32_t d_mlp;
  int32_t d_vocab;
  int32_t rotary_dim;
  int32_t n_ctx;       /* rotary table length */
  float ln_eps;
  float rotary_base;
} tvr_config;

/* Per-layer weights after TransformerLens processing (fold_ln,
 * center_writing_weights, fold_value_biases), in the engine's fused layout.
 *   w1 [3*d_model + d_mlp][d_model]  rows: Q(head,d_head) | K | V | MLP-in
 *   b1 [3*d_model + d_mlp]           (V part is zero after fold_value_biases)
 *   w2 [d_model][d_model + d_mlp]    cols: O(head,d_head) | MLP-out
 *   b2 [d_model]                     b_O (with folded value bias) + b_out   */
typedef struct tvr_layer_weights {
  const float* w1;
  const float* b1;
  const float* w2;
  const float* b2;
} tvr_layer_weights;

/* One patched forward = one (prompt, patch site) pair = one unit of the
 * metric "patched-forward prompts/sec". */
typedef struct tvr_site {
  int32_t seq;      /* clean sequence (prompt) index in the trace */
  int32_t kind;     /* enum tvr_site_kind */
  int32_t layer;    /* hook layer */
  int32_t head;     /* REPLACE_HEAD_ALLPOS */
  int32_t pos;      /* SET_RESID_PRE_POS / _VEC: patched position in `seq` (>= 0) */
  int32_t src_seq;  /* SET_RESID_PRE_POS: sequence supplying the row */
  int32_t src_pos;  /* SET_RESID_PRE_POS: position supplying the row */
  int32_t vec;      /* row of `vectors` (REPLACE / ADD / SET_RESID_PRE_VEC) */
  int32_t target;   /* token whose probability is reported, -1: none */
} tvr_site;

typedef struct tvr_model tvr_model;
typedef struct tvr_trace tvr_trace;

const char* tvr_version(void);
int32_t tvr_abi_version(void);
const char* tvr_last_error(void);

/* Replaces HookedTransformer.from_pretrained(...) (scratch.py:26,
 * scratch2.py:26): binds processed device weights (caller keeps them alive). */
int tvr_model_create(const tvr_config* cfg, const float* w_embed /*[V][d]*/,
                     const tvr_layer_weights* layers /*[n_layers] host*/,
                     const float* w_unembed_t /*[V][d]*/,
                     const float* b_unembed /*[V]*/, tvr_model** out);
int tvr_model_destroy(tvr_model* model);

/* Matrix-core path of the model's GEMMs (every other op is fp32 regardless).
 *   TVR_GEMM_F32     v_mfma_f32_32x32x2_f32 on the fp32 weights
 *   TVR_GEMM_X3BF16  fp32-accurate 3-plane bf16 split on v_mfma_f32_32x32x16_bf16:
 *                    each operand x = x0+x1+x2 (bf16 planes, 24 significand bits),
 *                    six cross products accumulated in fp32; weight planes 6 B/param
 *   TVR_GEMM_X2F16   fp32-accurate 2-plane fp16 split on v_mfma_f32_16x16x32_f16
 *                    (the fp16 form of 3xTF32): x = x0+x1 (2 x 11 significand
 *                    bits, power-of-two scaled into fp16 range), three cross
 *                    products accumulated in fp32; weight planes 4 B/param.
 *                    GEMM inputs must satisfy |a| < 4095 (LayerNorm outputs,
 *                    attention mixes and GELU outputs of any Pythia do); a
 *                    launch that sees a larger one is reported by
 *                    tvr_model_range_status.
 *   TVR_GEMM_BF16    bf16 weights and GEMM inputs on v_mfma_f32_16x16x32_bf16,
 *                    fp32 accumulation (the north star's bf16 configuration,
 *                    tolerance 2e-2; NOT fp32-accurate); weights 2 B/param.
 * Measured errors of both split modes against fp64 are at or below the fp32
 * MFMA GEMM's.  TransformerLens runs its matmuls in fp32
 * (scratch2.py:26 loads the default dtype); F32, X3BF16 and X2F16 meet that.
 * Everything outside the GEMMs (LayerNorm, attention, residual stream,
 * softmax) is fp32 in every mode.  The planes are built on the device once.
 * Synchronises `stream`. */
enum tvr_gemm_mode { TVR_GEMM_F32 = 0, TVR_GEMM_X3BF16 = 1, TVR_GEMM_X2F16 = 2, TVR_GEMM_BF16 = 3 };
int tvr_model_set_gemm(tvr_model* model, int32_t mode, void* stream);
int32_t tvr_model_get_gemm(const tvr_model* model);
/* TVR_OK, or TVR_ERR_RANGE if an X2F16 GEMM enqueued since the last call saw
 * an input outside its range (its results are then not fp32-accurate and must
 * be discarded).  Synchronises `stream`; clears the flag. */
int tvr_model_range_status(tvr_model* model, void* stream);

/* Exact-fp16 weights (the checkpoint dtype of every Pythia), for TVR_GEMM_X2F16.
 * Per layer, caller-owned device arrays, kept alive by the caller:
 *   w1  fp16 [3d + d_mlp][d]  the checkpoint's Q | K | V rows (engine order, as
 *                             tvr_layer_weights.w1) and MLP-in rows BEFORE fold_ln
 *   w2  fp16 [d][d + d_mlp]   W_O | W_out BEFORE center_writing_weights
 *   g1, g2 fp32 [d]           LN1 / LN2 gamma (ln_1.w, ln_2.w)
 * They must be the raw tensors the model's processed w1 / w2 were made from
 * (tvr_layer_weights: fold_ln, centring and fold_value_biases applied to them).
 * In X2F16 mode the QKV + MLP-in GEMM then reads LNPre(x) * gamma1 (Q, K, V
 * columns) and * gamma2 (MLP-in columns) against w1 — fold_ln's centring of the
 * read-in weights is a no-op on a centred LNPre row — and the O + MLP-out GEMM
 * reads w2 uncentred: the residual stream then carries one constant per row,
 * which every LayerNorm removes and tvr_trace_read's hook_resid_pre export
 * subtracts.  Weights exact in fp16 need 2 matrix products per 32-deep slice
 * instead of 3.  Results equal the processed-weight path's to fp32 rounding.
 * Pass layers == NULL to detach.  Other modes ignore the binding. */
typedef struct {
  const uint16_t* w1;
  const uint16_t* w2;
  const float* g1;
  const float* g2;
} tvr_exact16_layer;
int tvr_model_set_exact16(tvr_model* model, const tvr_exact16_layer* layers /*[n_layers] host, or NULL*/);
/* The unembed's part of the exact-fp16 binding (X2F16 mode, with the layers
 * bound): wu fp16 [d_vocab][d_model] = the checkpoint's embed_out.weight
 * BEFORE fold_ln / center_unembed, gf fp32 [d_model] = the final LN's gamma.
 * The patch sweeps' fused-statistics unembed then reads LNPre(x) * gf against
 * wu (2 products); the omitted centring over the vocabulary is one constant per
 * row of logits, which softmax probabilities and top-k do not see.  Paths that
 * return logits keep the processed W_U.  NULL, NULL detaches. */
int tvr_model_set_exact16_unembed(tvr_model* model, const uint16_t* wu, const float* gf);
/* Weight layout of the exact-fp16 GEMMs.  While the exact-fp16 path runs (X2F16
 * mode, layers bound) the engine keeps its own row-pair-interleaved copy
 * (tvr_weight_rows_il) of every bound w1, w2 and wu on the current device, and
 * the one-plane GEMMs read the copies: a staged weight piece is then 8 whole
 * 128-byte lines instead of 16 half lines.  Same values, same products in the
 * same order: bitwise the same results.  Cost: +2 bytes per bound parameter
 * (about 5.3 GB at Pythia-2.8B, 23 GB at 12B); the caller's planes stay bound,
 * are still read by everything but those GEMMs, and must stay alive.  The
 * copies are rebuilt on a rebind and freed on a detach, on a change to another
 * GEMM mode and with the model.  A copy that does not fit is no error: the
 * model runs on the plain planes and TVR_W_IL_NOMEM is reported here.
 * TVR_W_LAYOUT=rows in the environment (read by tvr_model_set_exact16 when the
 * layers are bound) keeps the plain planes everywhere; so do
 * TVR_ACT_LAYOUT=planar and engine builds without the wide one-plane tile.
 * Returns a mask of the flags below (0: plain planes everywhere), -1 for a null
 * model.  (Backward-compatible addition: ABI 11.) */
#define TVR_W_IL_LAYERS 1  /* w1 / w2 of every layer are read interleaved */
#define TVR_W_IL_UNEMBED 2 /* wu is read interleaved */
#define TVR_W_IL_NOMEM 4   /* a copy did not fit: its GEMMs read the plain plane */
int32_t tvr_model_weight_layout(const tvr_model* model);

/* Clean-run trace: every layer's hook_resid_pre, attn.hook_z and the K/V
 * inputs, the state run_with_cache keeps (scratch2.py:96, scratch.py:132,137). */
int tvr_trace_create(tvr_model* model, int32_t max_seqs, int32_t max_tokens,
                     tvr_trace** out);
/* Destroying a trace with a deferred clean forward pending runs it first (on
 * the null stream) so the caller's out_prob / out_topk are written. */
int tvr_trace_destroy(tvr_trace* trace);
/* Run a pending deferred clean forward now (tvr_forward_clean_deferred) on
 * `stream`; no-op otherwise. */
int tvr_trace_flush(tvr_trace* trace, void* stream);
/* Copy a traced hook into a caller device buffer [n_tokens][d] (async on
 * `stream`): what = TVR_TRACE_RESID_PRE gives blocks.{layer}.hook_resid_pre
 * (layer == n_layers: the final residual), TVR_TRACE_Z blocks.{layer}.attn.hook_z.
 * dst needs only float alignment (4 B).
 * TVR_TRACE_Q / _K / _V give blocks.{layer}.attn.hook_q / hook_k / hook_v
 * flattened over heads, BEFORE rotary (TransformerLens' hook_q, not hook_rot_q),
 * layer in [0, n_layers): the Q | K | V columns the layer's GEMM wrote on the
 * model's GEMM path, copied out of the trace's [tokens][3 d] rows.  hook_v
 * carries b_V = 0, as in the processed model (fold_value_biases).
 * (Backward-compatible addition: ABI 11.) */
enum tvr_trace_hook { TVR_TRACE_RESID_PRE = 0, TVR_TRACE_Z = 1, TVR_TRACE_Q = 2, TVR_TRACE_K = 3, TVR_TRACE_V = 4 };
int tvr_trace_read(const tvr_trace* trace, int32_t what, int32_t layer, float* dst,
                   void* stream);
int32_t tvr_trace_num_tokens(const tvr_trace* trace);
/* Grouped residual capture (Hendel et al.'s task-vector extraction):
 * out[g][l][:] += sum over sequences s with group[s] == g of
 * blocks.{l}.hook_resid_pre[row(s)]  (l == n_layers: the final residual),
 * row(s) = seq_off[s] + (pos ? pos[s] : seq_len[s] - 1), every l in [0, n_layers]
 * in one launch sequence.  Values are TransformerLens' (centred): on a trace
 * filled on the exact-fp16 path the per-row constant is removed, as
 * tvr_trace_read does.  pos host [n_seq] or NULL (last position); group host
 * [n_seq] in [0, n_groups) or NULL (one group); out device
 * [n_groups][n_layers + 1][d] fp32, float alignment (4 B) suffices: it is read
 * and written element-wise.  A group without sequences leaves its rows of out
 * untouched.  Runs a pending deferred clean forward first.  Sums run in a fixed
 * order that depends only on the group's sequence list (chunks of 16
 * sequences in sequence order, then the chunks in order), never on the launch
 * geometry: results are bitwise reproducible for a given trace.  group =
 * identity gives per-prompt vectors, n_groups = n_tasks many tasks from one
 * forward.  All arguments are validated before any device call:
 * TVR_ERR_INVALID for a null trace or out, an empty trace, a pos outside
 * [0, seq_len), a group outside [0, n_groups), n_groups <= 0.
 * (Backward-compatible addition: ABI 11.) */
int tvr_trace_capture_resid(tvr_trace* trace, const int32_t* pos, const int32_t* group,
                            int32_t n_groups, float* out, void* stream);
/* Attention patterns of one query per traced sequence, every layer and head in
 * one launch: out_pattern[s][l][h][j] = blocks.{l}.attn.hook_pattern[0, h, q, j]
 * of sequence s for q = pos ? pos[s] : seq_len[s] - 1 and keys j in [0, q];
 * columns (q, ld) are written as +0.0.  The pattern is the softmax over the keys
 * j <= q of rot(Q[q, h]) . rot(K[j, h]) / sqrt(d_head), computed in fp32 from
 * the Q / K rows the trace holds (TVR_TRACE_Q / _K: those of the model's GEMM
 * path, whichever it is) with the model's rotary tables.
 *   cls       host [n_tokens] class id per traced token in [-1, n_classes), or
 *             NULL; n_classes in [1, 64] when cls is given
 *   out_mass  device [n_seq][L][H][n_classes] or NULL (needs cls):
 *             out_mass[s][l][h][c] = sum over keys j <= q of sequence s with
 *             class c of the pattern (a key of class -1 is counted nowhere; a
 *             class without keys gives +0.0).  Todd et al.'s cheap head signal:
 *             where the last token attends, by token role.
 *   out_pattern device [n_seq][L][H][ld] or NULL, ld > the largest q
 * Both outputs are written element-wise: float alignment (4 B) suffices.
 * Sums run in a fixed order (a lane's keys in key order, then a fixed lane
 * tree), no atomics: results are bitwise reproducible for a given trace, and
 * the pattern's bits do not depend on whether the mass is requested.  Runs a
 * pending deferred clean forward first; everything is enqueued on `stream`.
 * Timed under TVR_HBM_ATTENTION.  All arguments are validated before any device
 * call: TVR_ERR_INVALID for a null trace, an empty trace, both outputs null,
 * out_mass without cls, n_classes outside [1, 64] with cls given, a class
 * outside [-1, n_classes), a pos outside [0, seq_len) or at or beyond n_ctx,
 * ld <= the largest q with out_pattern given.  TVR_ERR_UNSUPPORTED (before any
 * launch) if the longest key range does not fit the kernel's LDS (n_ctx beyond
 * about 16,000).  (Backward-compatible addition: ABI 11.) */
int tvr_trace_capture_pattern(tvr_trace* trace, const int32_t* pos, const int32_t* cls, int32_t n_classes,
                              float* out_pattern, int32_t ld, float* out_mass, void* stream);

/* Direct logit attribution at one query position per traced sequence, every layer and head from one clean
 * trace (TransformerLens: cache.stack_head_results / accumulated_resid, apply_ln_to_stack, logit_attrs).
 *   q        = pos ? pos[s] : seq_len[s] - 1
 *   x_l      = blocks.{l}.hook_resid_pre[q] of sequence s, x_L the final residual
 *   sigma_s  = sqrt(mean((x_L - mean x_L)^2) + ln_eps)
 *   u_s      = W_U'[:, target[s]] - W_U'[:, contrast[s]] (contrast NULL: W_U'[:, target[s]]), W_U' the processed
 *              w_unembed_t
 *   out_resid[s][l]   = (x_l - mean x_l) . u_s / sigma_s      device [n_seq][L + 1] or NULL; row 0 is the
 *              embedding's share, row L equals logit[target] - logit[contrast] minus the same difference of
 *              b_unembed
 *   out_head[s][l][h] = (z_l[q][h] @ W_O[l][h]) . u_s / sigma_s   device [n_seq][L][H] or NULL
 * pos, target, contrast: host [n_seq].  The row mean is always subtracted (a trace filled on the exact-fp16
 * path carries one constant per row, and u is mean-free only in exact arithmetic), computed as
 * tvr_trace_read's centred export computes it.  W_O is the processed fp32 tvr_layer_weights.w2 columns
 * [0, d) on every GEMM path.  Both outputs are written element-wise (float alignment).  Sums run in a fixed
 * order, no atomics: out_head[s][l][h] depends bit for bit only on sequence s' rows, l and h, not on n_seq.
 * Runs a pending deferred clean forward first; everything is enqueued on `stream`.  Timed under
 * TVR_HBM_CAPTURE (two spans: the direction pass, the head pass).  All arguments are validated before any
 * device call: TVR_ERR_INVALID for a null trace or target, both outputs null, an empty trace, a pos outside
 * its sequence, a target or contrast outside [0, d_vocab).  (Backward-compatible addition: ABI 11.) */
int tvr_trace_logit_attribution(tvr_trace* trace, const int32_t* pos, const int32_t* target,
                                const int32_t* contrast, float* out_head, float* out_resid, void* stream);
/* Per-source-token logit attribution of every head at one query position per traced sequence: FROM WHICH KEYS a
 * head carries the answer's logit, the product of tvr_trace_capture_pattern and tvr_trace_logit_attribution.
 * b_V is zero in the processed model (the trace's hook_v carries none), so hook_z[q, h] = sum_j p[j] v[j, h] and
 *   out_src[s][l][h][j] = p_l,h[q, j] * ((v_l[j, h] @ W_O[l][h]) . u_s / sigma_s)     j in [0, q]
 *   sum over j of out_src[s][l][h][j] = out_head[s][l][h] of tvr_trace_logit_attribution
 * with q, u_s, sigma_s as tvr_trace_logit_attribution defines them and p the pattern of
 * tvr_trace_capture_pattern, recomputed with that kernel's arithmetic (the same bits); columns (q, ld) are
 * written as +0.0.
 *   pos, target, contrast  host [n_seq]; pos and contrast may be NULL
 *   cls      host [n_tokens] class id per traced token in [-1, n_classes), or NULL; n_classes in [1, 64] when
 *            cls is given
 *   out_src  device [n_seq][L][H][ld] or NULL, ld > the largest q
 *   out_cls  device [n_seq][L][H][n_classes] or NULL (needs cls): out_cls[s][l][h][c] = sum over keys j <= q of
 *            sequence s with class c of out_src[s][l][h][j] (a key of class -1 is counted nowhere; a class
 *            without keys gives +0.0)
 * Both outputs are written element-wise: float alignment (4 B) suffices.  Three kernels: the direction pass of
 * tvr_trace_logit_attribution; the G pass of tvr_head_directions (g = dirs W_O, so that
 * (v_j @ W_O[h]) . dirs = v_j[h] . g); the source kernel of tvr_attention_source over the trace's Q / K / V rows.
 * The last two run in groups of layers whose [layers][n_seq][d] G buffer stays within 64 MiB of the model's
 * workspace (one layer at least); the grouping cannot change a bit.  Sums run in a fixed order, no atomics:
 * out_src[s][l][h][:] depends bit for bit only on sequence s' rows, l and h, not on n_seq, and not on whether
 * out_cls is requested.  W_O is the processed fp32 tvr_layer_weights.w2 columns [0, d) on every GEMM path.  Runs
 * a pending deferred clean forward first; everything is enqueued on `stream`.  Timed under TVR_HBM_CAPTURE (the
 * direction pass, the G pass per group) and TVR_HBM_ATTENTION (the source kernel per group).  All arguments are
 * validated before any device call: TVR_ERR_INVALID for a null trace or target, an empty trace, both outputs null,
 * out_cls without cls, n_classes outside [1, 64] with cls given, a class outside [-1, n_classes), a pos outside
 * [0, seq_len) or at or beyond n_ctx, a target or contrast outside [0, d_vocab), ld <= the largest q with out_src
 * given.  TVR_ERR_UNSUPPORTED (before any launch) if the longest key range does not fit the kernel's 64 KiB of
 * LDS.  (Backward-compatible addition: ABI 11.) */
int tvr_trace_source_attribution(tvr_trace* trace, const int32_t* pos, const int32_t* target, const int32_t* contrast,
                                 const int32_t* cls, int32_t n_classes, float* out_src, int32_t ld, float* out_cls,
                                 void* stream);
/* Logit lens: every layer's residual row at the query position through the final LayerNormPre and the
 * unembedding, out index [s][l], l in [0, L] (l == L: the model's own last-layer distribution at q).
 * Row l of sequence s is gathered from the trace in place.  targets host [n_seq] or NULL; out_prob device
 * [n_seq][L + 1] = softmax(logits)[targets[s]] or NULL (needs targets); out_topk device [n_seq][L + 1][topk]
 * int32 (descending, lowest id on ties) or NULL; topk in [1, 16] with out_topk (else ignored, in [0, 16]).
 * The rows take tvr_forward_clean's final stage as it is: LNPre with each row's own scale, the unembed with
 * the fused statistics on the model's GEMM path (the exact-fp16 unembed where bound).  Runs a pending
 * deferred clean forward first.  TVR_ERR_INVALID for a null or empty trace, no output at all, out_prob
 * without targets, a bad topk, a pos outside its sequence, a target outside [0, d_vocab); validated before
 * any device call.  (Backward-compatible addition: ABI 11.) */
int tvr_trace_logit_lens(tvr_trace* trace, const int32_t* pos, const int32_t* targets, float* out_prob,
                         int32_t* out_topk, int32_t topk, void* stream);

/* Batched clean forward of n_seq prompts (ragged lengths, packed tokens).
 * Replaces the per-prompt model.forward / run_with_cache calls
 * (scratch2.py:96,143,183,297; scratch.py:127,132,137).
 *   trace        may be NULL (no snapshots kept)
 *   targets      host [n_seq] token ids or NULL; out_prob [n_seq] gets
 *                softmax(logits[-1])[target]
 *   out_topk     device [n_seq][topk] int32 (descending, lowest id on ties)
 *   out_logits   device [n_seq][V] last-position logits, or NULL
 *   capture_zsum device [n_layers][d] fp32: += hook_z at each prompt's last
 *                position (the reduction of scratch2.py:97-98), or NULL   */
int tvr_forward_clean(tvr_model* model, tvr_trace* trace, const int32_t* tokens,
                      const int32_t* seq_lens, int32_t n_seq,
                      const int32_t* targets, float* out_prob,
                      int32_t* out_topk, int32_t topk, float* out_logits,
                      float* capture_zsum, void* stream);

/* tvr_forward_clean (no logits, no capture) deferred into the next
 * tvr_patch_sweep on `trace`: that sweep runs the clean rows in its own
 * launches (one staircase instead of a clean forward + a staircase), fills the
 * trace exactly as tvr_forward_clean would, and writes out_prob / out_topk
 * (stream-ordered: read them after that sweep).  Any other use of the trace
 * first (tvr_trace_read, tvr_forward_clean, another deferral) runs the clean
 * forward on its own.  Same checks and errors as tvr_forward_clean; no GPU
 * work is enqueued by this call.  The reference's pattern it serves: a clean
 * forward and the patched forwards of the same prompts (scratch2.py:143-148,
 * 183-192). */
int tvr_forward_clean_deferred(tvr_model* model, tvr_trace* trace, const int32_t* tokens,
                               const int32_t* seq_lens, int32_t n_seq,
                               const int32_t* targets, float* out_prob,
                               int32_t* out_topk, int32_t topk, void* stream);

/* Logits of EVERY position, out_logits device [sum(seq_lens)][V]: the
 * TransformerLens forward's [1, T, V] (scratch2.py:143,183,297;
 * scratch.py:127,143).  Exactly one input:
 *   tokens   host ids (packed, seq_lens per sequence), start_layer 0, or
 *   resid_in device [sum(seq_lens)][d] = blocks.{start_layer}.hook_resid_pre,
 *            continued from that block (forward(resid, start_at_layer=L),
 *            scratch.py:143,206,209).
 * Sequences up to n_ctx tokens (beyond 128 the attention runs its chunked
 * online-softmax form). */
int tvr_forward_logits(tvr_model* model, const int32_t* tokens, const float* resid_in,
                       int32_t start_layer, const int32_t* seq_lens, int32_t n_seq,
                       float* out_logits, void* stream);

/* Batched patch sweep over sites against a clean trace (the staircase: a site
 * at layer l reuses the clean run's layers <= l and K/V prefix).  Replaces the
 * per-site run_with_hooks loops (scratch2.py:122-125,145-148,185-194,301,311;
 * scratch.py:140-145).
 *   vectors  device [n_vectors][d]
 *   out_prob device [n_sites], out_topk device [n_sites][topk],
 *   out_logits device [n_sites][V] or NULL                                  */
int tvr_patch_sweep(tvr_model* model, tvr_trace* trace,
                    const tvr_site* sites, int32_t n_sites,
                    const float* vectors, int32_t n_vectors, float* out_prob,
                    int32_t* out_topk, int32_t topk, float* out_logits,
                    void* stream);
/* (tvr_patch_sweep takes kinds 0-3 and 6; it rejects the head-set kinds 4 and 5
 * with TVR_ERR_INVALID and a message naming tvr_patch_sweep_sets.) */

/* tvr_patch_sweep with head-set sites: one patched forward replaces the
 * hook_result of a SET of (layer, head) pairs at once — the joint mean-ablation
 * / joint patching of the function-vector paper, which the reference side
 * writes as one run_with_hooks call with one scratch2.py:188 hook per member.
 *   set_off  host [n_sites + 1], non-decreasing, set_off[0] >= 0: a site of
 *            kind TVR_SITE_REPLACE_HEADSET_ALLPOS / _LASTPOS owns
 *            patches[set_off[i] .. set_off[i+1]); a site of kinds 0-3 or 6 must own
 *            an empty range and behaves exactly as in tvr_patch_sweep (mixed
 *            launches are fine).  An empty set equals TVR_SITE_NONE.
 *   patches  host [set_off[n_sites]] (the caller guarantees that length; may be
 *            NULL when every set is empty).  layer in [0, n_layers), head in
 *            [0, n_heads), vec in [0, n_vectors); the same (layer, head) twice
 *            in one set is an error.  The vectors of one (site, layer) are
 *            summed in list order (fp32), so results are reproducible bit for
 *            bit for a given list.
 *   vectors  device [n_vectors][d], any vectors (not only ones in the row
 *            space of W_O[head]): head h of layer l is replaced by zeroing its
 *            d_head columns of that layer's O-projection input and adding the
 *            vector to the residual rows the projection accumulates into.
 *            Alignment: for the head-set kinds float (4 B) suffices — a base
 *            that is not 16-byte aligned takes an element-wise variant of the
 *            head-set kernel instead of the float4 one.  The kernels of
 *            TVR_SITE_REPLACE_HEAD_ALLPOS read `vectors` with 16-byte loads:
 *            a launch that holds such a site with a base that is not 16-byte
 *            aligned returns TVR_ERR_INVALID here (tvr_patch_sweep does not
 *            check: pass it a 16-byte aligned base; the test primitive
 *            tvr_site_entry does check, with or without sets).  TVR_SITE_SET_RESID_PRE_VEC
 *            reads it element-wise: float alignment suffices in both sweeps.
 * A set site enters the staircase at its lowest patched layer and computes
 * every layer from there (ALLPOS: all T rows; LASTPOS: the last row, against
 * the clean K/V).  Works on a filled trace and on a deferred clean forward, on
 * every GEMM path.  All arguments are validated before any device call:
 * TVR_ERR_INVALID for null arguments, decreasing offsets, a layer / head / vec
 * out of range, a duplicate (layer, head), patches owned by a site of kinds 0-3.
 * Outputs as tvr_patch_sweep.  (Backward-compatible addition: ABI 11.) */
typedef struct tvr_head_patch { int32_t layer, head, vec; } tvr_head_patch;
int tvr_patch_sweep_sets(tvr_model* model, tvr_trace* trace,
                         const tvr_site* sites, int32_t n_sites,
                         const int32_t* set_off, const tvr_head_patch* patches,
                         const float* vectors, int32_t n_vectors, float* out_prob,
                         int32_t* out_topk, int32_t topk, float* out_logits,
                         void* stream);

/* tvr_patch_sweep_sets with attention-knockout sites (Geva et al. 2023; Wang et
 * al. 2023): cut the edges from a prompt's last position to chosen key
 * positions in chosen (layer, head) pairs and re-measure the answer.
 *   set_off, patches  as tvr_patch_sweep_sets.  A site of kind
 *            TVR_SITE_ATTN_KNOCKOUT_LASTPOS owns patches[set_off[i] .. set_off[i+1])
 *            as its (layer, head) members; their `vec` is ignored (-1 is fine);
 *            the same (layer, head) twice is an error.
 *   key_off  host [n_sites + 1], non-decreasing, key_off[0] >= 0: a kind-7 site
 *            owns keys[key_off[i] .. key_off[i+1]); every other kind owns an
 *            empty range (kinds 4 / 5 keep their patches, kinds 0-3 and 6 own
 *            neither).  Mixed launches are fine.
 *   keys     host int32 [key_off[n_sites]] (may be NULL when every range is
 *            empty): per site strictly increasing positions in [0, seq_len - 1],
 *            fewer than seq_len of them — one key of the last query must remain,
 *            so the engine never divides by an empty softmax.
 *   vectors  may be NULL when no site reads one.
 * A kind-7 site is planned as TVR_SITE_REPLACE_HEADSET_LASTPOS: it enters at its
 * lowest member layer as a copy of its clean last row and computes that one row
 * of every later layer against the clean K/V; at each layer where it has members
 * one launch (attention_knockout_kernel, timed under TVR_HBM_ATTENTION)
 * recomputes their z slices between the attention and the O + MLP-out GEMM.  A
 * site with no members or no keys equals TVR_SITE_NONE bit for bit and adds no
 * launch; a sweep without kind-7 sites enqueues what tvr_patch_sweep_sets does.
 * Works on a filled trace and on a deferred clean forward, on every GEMM path,
 * with exact-fp16 weights bound or not.  All arguments are validated before any
 * device call: TVR_ERR_INVALID for what tvr_patch_sweep_sets refuses, null or
 * decreasing key_off, null keys with a non-empty range, keys owned by another
 * kind, a key out of range or out of order, every key blocked;
 * TVR_ERR_UNSUPPORTED for a model with more than 64 heads (the head mask) or a
 * sequence whose scores do not fit the kernel's LDS.  Outputs as
 * tvr_patch_sweep.  tvr_patch_sweep and tvr_patch_sweep_sets reject kind 7
 * ("unknown kind").  (Backward-compatible addition: ABI 11.) */
int tvr_patch_sweep_knockout(tvr_model* model, tvr_trace* trace,
                             const tvr_site* sites, int32_t n_sites,
                             const int32_t* set_off, const tvr_head_patch* patches,
                             const int32_t* key_off, const int32_t* keys,
                             const float* vectors, int32_t n_vectors, float* out_prob,
                             int32_t* out_topk, int32_t topk, float* out_logits,
                             void* stream);

/* out[l][h][:] = zsum[l][h*d_head:(h+1)*d_head] @ W_O[l,h]: turns the z-form
 * capture into the hook_result form of scratch2.py:98 (sum over prompts). */
int tvr_project_heads(tvr_model* model, const float* zsum /*[L][d]*/,
                      float* out /*[L][H][d]*/, void* stream);

/* Primitive kernels, exported for unit tests and tools. */
/* C[M][N] = A[M][K] (row stride lda) @ W[N][K]^T (row stride ldw) + bias */
int tvr_gemm_f32(const float* A, int32_t lda, const float* W, int32_t ldw,
                 const float* bias, float* C, int32_t ldc, int32_t M,
                 int32_t N, int32_t K, void* stream);
/* Split W [n] fp32 into 3 bf16 planes out [3][n] (uint16 storage). */
int tvr_split_planes(const float* w, uint16_t* out, size_t n, void* stream);
/* tvr_gemm_f32 on the 3-plane operand: W planes [3][.][ldw] with plane
 * stride wps elements (as tvr_split_planes writes them, wps = n). */
int tvr_gemm_x3bf16(const float* A, int32_t lda, const uint16_t* W, int32_t ldw,
                    size_t wps, const float* bias, float* C, int32_t ldc,
                    int32_t M, int32_t N, int32_t K, void* stream);
/* Weight planes of a planar mode (fmt = TVR_GEMM_X2F16 or TVR_GEMM_BF16):
 * X2F16 two fp16 planes out [2][n] of w * scale (scale a power of two; the
 * engine uses 2^(15 - ceil log2 max|W|)), BF16 one bf16 plane out [n]. */
int tvr_weight_planes(int32_t fmt, const float* w, float scale, uint16_t* out, size_t n,
                      void* stream);
/* tvr_gemm_f32 with the split happening inside the GEMM: A fp32, W planes
 * [2][.][ldw] (plane stride wps) from tvr_weight_planes(TVR_GEMM_X2F16, ..,
 * w_scale, ..).  *range_flag (device, may be NULL) is or-ed with 1 if |A|
 * reaches the split's range limit. */
int tvr_gemm_x2f16(const float* A, int32_t lda, const uint16_t* W, int32_t ldw,
                   size_t wps, float w_scale, const float* bias, float* C,
                   int32_t ldc, int32_t M, int32_t N, int32_t K,
                   uint32_t* range_flag, void* stream);
/* The activation format the engine's producers write for every GEMM input in
 * a planar mode: logical [rows][K] -> halves [rows][2][K]; X2F16: plane 0 =
 * fp16(16 a), plane 1 = fp16(16 a - plane 0), *range_flag (may be NULL) |= 1
 * if |a| >= 4095; BF16: plane 0 = bf16(a).
 * fmt = TVR_ACT_X2F16_IL (K % 32 == 0): the X2F16 values in the k-tile-
 * interleaved layout the exact-fp16 sweeps use internally, halves
 * [rows][K / 32][2][32] — per row and 32-column group, 64 B of plane 0 then
 * 64 B of plane 1 (one 128-B line): column c of plane p is half
 * (c / 32) * 64 + p * 32 + c % 32 of the row.  Same values, same bytes per
 * row (2 K halves), same range flag. */
#define TVR_ACT_X2F16_IL 0x12 /* TVR_GEMM_X2F16 | 0x10 */
int tvr_act_rows(int32_t fmt, const float* a, int32_t lda, uint16_t* out, int32_t rows,
                 int32_t K, uint32_t* range_flag, void* stream);
/* One fp16 weight plane w [N][K] (K % 32 == 0) in the row-pair-interleaved
 * layout of the exact-fp16 GEMMs, halves [ceil(N / 2)][K / 32][2][32]: rows
 * 2 p and 2 p + 1 share pair p, and per pair and 32-column group 64 B of the
 * even row are followed by 64 B of the odd row (one 128-B line) — element
 * (n, k) is half (n / 2) * 2 K + (k / 32) * 64 + (n % 2) * 32 + k % 32.  out
 * holds ceil(N / 2) * 2 K halves; the missing partner row of an odd N is
 * written as zeros.  The layout tvr_gemm_launch's exact16 = 2 reads.
 * TVR_ERR_INVALID for a null w / out, N or K <= 0, K % 32 != 0.  Enqueues on
 * `stream` without synchronising.  (Backward-compatible addition: ABI 11.) */
int tvr_weight_rows_il(const uint16_t* w, uint16_t* out, int32_t N, int32_t K, void* stream);
/* The engine's planar GEMM: A in the activation format above (lda logical
 * elements per row, >= K), W planes from tvr_weight_planes (w_scale: the
 * X2F16 scale, 1 for BF16).  fmt = TVR_ACT_X2F16_IL: A in the interleaved
 * layout (row stride 2 lda halves), the X2F16 weight planes; the same
 * products in the same order as TVR_GEMM_X2F16 — bitwise the same C. */
int tvr_gemm_planar(int32_t fmt, const uint16_t* A, int32_t lda, const uint16_t* W,
                    int32_t ldw, size_t wps, float w_scale, const float* bias,
                    float* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                    void* stream);
/* TransformerLens LayerNormPre over rows: (x - mean) / sqrt(var + eps) */
int tvr_lnpre_f32(const float* x, int32_t ldx, float* y, int32_t ldy,
                  int32_t rows, int32_t d, float eps, void* stream);
/* One LayerNormPre launch exactly as the engine makes it (engine.hip
 * launch_lnpre: the row in registers for d % 256 == 0 up to 5120, else three
 * passes), on a caller's buffers, with every option a block or the unembed uses:
 *   x, ldx, x_rows   device fp32 [x_rows][ldx]; launch row r reads row
 *            row_idx[r] (row_idx host [rows], copied to a temporary device
 *            buffer), or row r with row_idx NULL (then rows <= x_rows)
 *   fmt      0: y is fp32 [rows][ldy]; TVR_GEMM_X2F16, TVR_ACT_X2F16_IL,
 *            TVR_GEMM_BF16: y is halves [rows][2 ldy] in the format tvr_act_rows
 *            describes (BF16: plane 1 holds fp16(y), the Q / K operands).  The
 *            interleaved layout addresses whole 32-column groups: d and ldy
 *            multiples of 32
 *   stats    device [rows][2] or NULL: (mean, sqrt(var + eps)) of launch row r
 *   copy, copy_rows  device [min(rows, copy_rows)][ldx] or NULL: launch rows
 *            r < copy_rows of x (after the gather) unchanged; copy_rows > rows
 *            means all rows
 *   g1, g2, y2  device [d] gammas, or NULL (x2f16 formats only): y = LNPre(x) g1
 *            and, with g2 and y2 (laid out as y), y2 = LNPre(x) g2; a value with
 *            |y| >= 4095 is reported by tvr_model_range_status of `model`
 *   model    may be NULL without g1
 * All arguments are validated on the host before any device call:
 * TVR_ERR_INVALID for null args / x / y, an unknown fmt, rows or x_rows <= 0, d,
 * ldx or ldy not positive multiples of 4, ldx < d or ldy < d, x, y, y2, copy or a
 * gamma not 16-byte aligned (stats: 8-byte), a row_idx entry outside
 * [0, x_rows) (rows > x_rows without row_idx), copy_rows < 0 or positive with
 * a NULL copy, g1 with fmt 0 or BF16 or with a NULL model, y2 without g1 and g2,
 * g2 without y2, and for TVR_ACT_X2F16_IL d or ldy not a multiple of 32.
 * A test primitive: it synchronises `stream`.  (Backward-compatible addition: ABI 11.) */
typedef struct tvr_lnpre_args {
  int32_t fmt, rows, d, ldx, ldy, x_rows, copy_rows;
  float eps;
  const float* x;
  const int32_t* row_idx;
  void* y;
  float* stats;
  float* copy;
  const float* g1;
  const float* g2;
  void* y2;
} tvr_lnpre_args;
int tvr_lnpre_rows(tvr_model* model, const tvr_lnpre_args* args, void* stream);
/* dst[r] = src[r] - mean(src[r]) over rows of d floats, device [rows][d], as the
 * engine centres the exact-fp16 path's logits (in place) and trace export: the
 * float4 kernel where src and dst are 16-byte aligned and d % 4 == 0, else the
 * element-wise one.  src == dst is allowed.  TVR_ERR_INVALID, before any device
 * call, for a null or not float-aligned src / dst, rows or d <= 0, or src and dst
 * overlapping without being equal.  A test primitive: it synchronises `stream`.
 * (Backward-compatible addition: ABI 11.) */
int tvr_center_rows(const float* src, float* dst, int32_t rows, int32_t d, void* stream);
/* The engine's causal attention of ragged sequences, launched exactly as a
 * block of the model launches it (the kernel form is chosen from the longest
 * p0 + n, TVR_ATT_STAGE / TVR_ATT_VSTAGE / TVR_ROW_ATTN and row_from).
 * A sequence computes the rows [row0, row0 + n) of qkv, the positions
 * [p0, p0 + n); the K / V rows of positions [0, p0) are rows cache_row .. of
 * `cache` (prefix_live 0) or of qkv itself (prefix_live 1: a leader's rows of
 * the same launch); rows [q0, n) are queries.  Sequences [row_from, n_seq)
 * have exactly one query (q0 = n - 1) and take the single-query kernel where
 * the model's n_heads allows it; row_from = n_seq: none.
 *   qkv    device [rows][3 d]: Q | K | V per row, before rotary
 *   cache  device [cache_rows][3 d] (its Q columns are not read), or NULL
 *   seqs   host [n_seq]
 *   fmt    0: z is fp32 [rows][K2], K2 = d_model + d_mlp; TVR_GEMM_X2F16,
 *          TVR_ACT_X2F16_IL, TVR_GEMM_BF16: z is halves [rows][2 K2] in the
 *          format tvr_act_rows describes (the layout of the engine's buffer
 *          for the O + MLP-out GEMM's input).  Only columns [0, d) of the
 *          query rows are written.
 *   zf     device fp32 [.][d] or NULL: a copy of z's query rows with row
 *          index < zf_rows (zf_last 0), or of sequence s' last row at row s
 *          (zf_last 1)
 *   cos_t, sin_t  device [n_ctx][d_head / 4] rotary tables (TransformerLens'
 *          calculate_sin_cos_rotary layout), or both NULL: the model's own
 * All arguments are validated on the host before any device call:
 * TVR_ERR_INVALID for a null model / qkv / z / seqs, n_seq <= 0, an unknown
 * fmt, a buffer that is not 16-byte aligned, one table without the other,
 * row_from outside [0, n_seq], rows <= 0, cache_rows < 0, zf_rows < 0, and
 * per sequence n < 1, q0 outside [0, n),
 * p0 < 0, p0 + n > n_ctx, rows outside [0, rows), with p0 > 0 a negative
 * cache_row, a prefix outside its buffer or a null cache, and q0 != n - 1 at or
 * after row_from.  A test primitive: it copies the descriptors to a temporary
 * device buffer and synchronises `stream`.  An x2f16 value with |z| >= 4095
 * is reported by tvr_model_range_status.  (Backward-compatible addition: ABI 11.) */
typedef struct tvr_attn_seq { int32_t row0, n, p0, cache_row, q0, prefix_live; } tvr_attn_seq;
int tvr_attention(tvr_model* model, int32_t fmt, const float* qkv, const float* cache,
                  const tvr_attn_seq* seqs, int32_t n_seq, int32_t row_from, int32_t rows,
                  int32_t cache_rows, void* z, float* zf, int32_t zf_last, int32_t zf_rows,
                  const float* cos_t, const float* sin_t, void* stream);
/* One knockout launch (what a layer of tvr_patch_sweep_knockout applies after
 * the attention) on a caller's buffers: for every item, the z slices of the
 * listed heads of sequence `seq`'s LAST row (row0 + n - 1, position p0 + n - 1)
 * are overwritten with the attention of that query over the keys that are not
 * blocked.  Nothing else of z is written.
 *   qkv, cache, seqs, rows, cache_rows, cos_t, sin_t   as tvr_attention (q0 is
 *          not read); the tables 16-byte aligned when given
 *   items  host [n_items]: sequence index, head mask (bit h: head h), and the
 *          range [first_key, first_key + n_keys) of `keys`: strictly increasing
 *          positions in [0, p0 + n), fewer than p0 + n of them.  An empty range
 *          recomputes the plain attention of the listed heads; heads = 0 writes
 *          nothing.  Two items must not list the same head of the same row.
 *   z      device, 16-byte aligned, in format fmt on tvr_attention's [rows][K2]
 *          layout
 * All arguments are validated on the host before any device call:
 * TVR_ERR_INVALID for a null model / qkv / z / seqs / items, n_seq <= 0,
 * n_items <= 0, n_keys < 0 or null keys with n_keys > 0, an unknown fmt,
 * misaligned buffers, one table without the other, every sequence as
 * tvr_attention checks it, an item whose seq, head mask or key range is out of
 * range, keys out of range or order, every key blocked, a (row, head) listed
 * twice; TVR_ERR_UNSUPPORTED for more than 64 heads or scores that do not fit
 * the LDS.  A test primitive: it copies the tables to a temporary device buffer
 * and synchronises `stream`.  An x2f16 value with |z| >= 4095 is reported by
 * tvr_model_range_status.  (Backward-compatible addition: ABI 11.) */
typedef struct tvr_knockout_item { int32_t seq; uint64_t heads; int32_t first_key, n_keys; } tvr_knockout_item;
int tvr_attention_knockout(tvr_model* model, int32_t fmt, const float* qkv, const float* cache,
                           const tvr_attn_seq* seqs, int32_t n_seq, int32_t rows, int32_t cache_rows,
                           const tvr_knockout_item* items, int32_t n_items, const int32_t* keys,
                           int32_t n_keys, void* z, const float* cos_t, const float* sin_t, void* stream);
/* The pattern kernel of tvr_trace_capture_pattern alone, on a caller's buffer
 * (one layer): sequence s is the positions 0 .. qpos[s] at rows row0[s] .. of
 * qkv, its query the row row0[s] + qpos[s].  Only the query row's Q columns and
 * the K columns of rows [row0, row0 + qpos] are read.
 *   qkv    device [rows][3 d]: Q | K | V per row, before rotary, 16-byte aligned
 *   cls    host [rows] (indexed by row) in [-1, n_classes), or NULL
 *   out_pattern device [n_seq][H][ld] or NULL; out_mass device
 *          [n_seq][H][n_classes] or NULL; written element-wise (float alignment)
 *   cos_t, sin_t  device [n_ctx][d_head / 4], 16-byte aligned, or both NULL:
 *          the model's own
 * TVR_ERR_INVALID as tvr_trace_capture_pattern, and for a null model / qkv /
 * row0 / qpos, n_seq <= 0, rows <= 0, a qpos outside [0, n_ctx), rows
 * [row0, row0 + qpos] outside the buffer, a qkv or table that is not 16-byte
 * aligned, one table without the other.  A test primitive: it copies the
 * descriptors to a temporary device buffer and synchronises `stream`.
 * (Backward-compatible addition: ABI 11.) */
int tvr_attention_pattern(tvr_model* model, const float* qkv, int32_t rows, const int32_t* row0,
                          const int32_t* qpos, int32_t n_seq, const int32_t* cls, int32_t n_classes,
                          float* out_pattern, int32_t ld, float* out_mass, const float* cos_t,
                          const float* sin_t, void* stream);
/* The head pass of tvr_trace_logit_attribution alone, on a caller's buffers (one layer): which heads write
 * along a direction.
 *   out[i][h] = (z[i][h*dh .. (h+1)*dh) @ W_O[layer][h]) . dirs[i]      i in [0, n)
 * z, dirs device [n][d], 16-byte aligned (else TVR_ERR_INVALID); out device [n][H], written element-wise
 * (float alignment); nothing outside [n][H] is written and no row beyond n is read.  W_O: the processed fp32
 * tvr_layer_weights.w2 columns [0, d), the operand of tvr_project_heads, on every GEMM path and with
 * exact-fp16 weights bound.  The bits of out[i][h] depend only on row i, the layer and the head.
 * TVR_ERR_INVALID for null arguments, n <= 0 or a layer out of range, before any device call.  Enqueues on
 * `stream` without synchronising.  (Backward-compatible addition: ABI 11.) */
int tvr_head_attribution(tvr_model* model, int32_t layer, const float* z, const float* dirs, int32_t n,
                         float* out, void* stream);
/* The G pass of tvr_trace_source_attribution alone, on a caller's buffers (one layer): a direction per row
 * pulled back through W_O into the heads' z coordinates.
 *   out_g[i][h*dh + k] = sum over c of dirs[i][c] * W_O[layer][c][h*dh + k]      i in [0, n)
 * so that (z @ W_O[layer][h]) . dirs[i] = z[h*dh .. (h+1)*dh) . out_g[i][h*dh .. (h+1)*dh).  dirs and out_g
 * device [n][d], 16-byte aligned (else TVR_ERR_INVALID); nothing outside [n][d] is written and no row beyond
 * n is read.  W_O: the processed fp32 tvr_layer_weights.w2 columns [0, d) on every GEMM path and with
 * exact-fp16 weights bound, as in tvr_head_attribution.  The bits of out_g[i][col] depend only on row i of
 * dirs, the layer and the column.  TVR_ERR_INVALID for null arguments, n <= 0, a layer out of range or a
 * misaligned buffer, before any device call.  Enqueues on `stream` without synchronising.  Timed under
 * TVR_HBM_CAPTURE.  (Backward-compatible addition: ABI 11.) */
int tvr_head_directions(tvr_model* model, int32_t layer, const float* dirs, int32_t n, float* out_g, void* stream);
/* The source kernel of tvr_trace_source_attribution alone, on a caller's buffer (one layer): sequence s is
 * the positions 0 .. qpos[s] at rows row0[s] .. of qkv, its query the row row0[s] + qpos[s].
 *   out_src[s][h][j] = p[j] * (V[row0[s] + j][h*dh .. (h+1)*dh) . g[s][h*dh .. (h+1)*dh))     j in [0, qpos[s]]
 * with p tvr_attention_pattern's pattern (the same bits); columns (qpos[s], ld) are written as +0.0.  Only
 * the query row's Q columns and the K and V columns of rows [row0, row0 + qpos] are read.
 *   qkv    device [rows][3 d]: Q | K | V per row, before rotary, 16-byte aligned
 *   g      device [n_seq][d], 16-byte aligned, required (tvr_head_directions' output for the sequences'
 *          directions)
 *   cls    host [rows] (indexed by row) in [-1, n_classes), or NULL
 *   out_src device [n_seq][H][ld] or NULL; out_cls device [n_seq][H][n_classes] or NULL (needs cls): the
 *          sums of out_src over the keys of each class; written element-wise (float alignment)
 *   cos_t, sin_t  device [n_ctx][d_head / 4], 16-byte aligned, or both NULL: the model's own
 * Argument rules and errors are tvr_attention_pattern's (with out_src / out_cls for out_pattern / out_mass),
 * and TVR_ERR_INVALID for a null or misaligned g.  TVR_ERR_UNSUPPORTED before any launch if the longest key
 * range does not fit the kernel's 64 KiB of LDS ((2 d_head + keys) floats).  A test primitive: it copies the
 * descriptors to a temporary device buffer and synchronises `stream`.
 * (Backward-compatible addition: ABI 11.) */
int tvr_attention_source(tvr_model* model, const float* qkv, int32_t rows, const int32_t* row0, const int32_t* qpos,
                         int32_t n_seq, const float* g, const int32_t* cls, int32_t n_classes, float* out_src,
                         int32_t ld, float* out_cls, const float* cos_t, const float* sin_t, void* stream);
/* Vocabulary decoding of any rows (task vectors, function vectors, residual rows): tvr_trace_logit_lens'
 * stage on a caller's buffer.  rows device [n][d], 16-byte aligned; targets host [n] or NULL; out_prob
 * device [n] or NULL; out_topk device [n][topk] or NULL; same rules and errors as tvr_trace_logit_lens, and
 * TVR_ERR_INVALID for a null model or rows, n <= 0 or rows not 16-byte aligned.
 * (Backward-compatible addition: ABI 11.) */
int tvr_decode_rows(tvr_model* model, const float* rows, int32_t n, const int32_t* targets, float* out_prob,
                    int32_t* out_topk, int32_t topk, void* stream);
/* One planar GEMM through the engine's own dispatch (engine.hip launch_gemm:
 * the skinny kernel, or gemm_pingpong_kernel plain, split over K, with a split
 * tail or stream-K and their reduce kernels, each picked by the selectors of
 * gemm_pingpong.hpp, pp_kernel / pp_reduce_kernel; a form they do not hold is
 * TVR_ERR_INTERNAL, which no checked argument reaches), C = A W^T under one
 * fused epilogue.  The
 * split-K workspace lives on the model; a tiny model is enough, its weights are
 * not used.
 *   fmt      TVR_GEMM_X2F16, TVR_ACT_X2F16_IL or TVR_GEMM_BF16: A (and a2) in
 *            the format tvr_act_rows describes, row stride 2 lda halves
 *   exact16  0: W planes from tvr_weight_planes (X2F16 [2][.][ldw], plane
 *            stride wps, of w * w_scale; BF16 one plane, w_scale unused);
 *            1: ONE fp16 plane of w * w_scale holding the weights exactly
 *            (x2f16 formats only: two products per slice).  The interleaved
 *            layout with two weight planes runs only the plain bias launch.
 *            2: as 1 with the plane row-pair interleaved (tvr_weight_rows_il
 *            with K = ldw: ceil(N / 2) pairs of 2 ldw halves, allocated by the
 *            caller); fmt TVR_ACT_X2F16_IL only, TVR_ERR_INVALID with any
 *            other; otherwise validated as 1; bitwise the results of 1.
 *   epi      TVR_EPI_BIAS   out0[r][c] = acc + bias[c]
 *            TVR_EPI_GELU   c < n_split as TVR_EPI_BIAS; else erf-GELU(acc +
 *                           bias) in the activation format (the layout follows
 *                           fmt) at out1h, row stride ld1h halves, column
 *                           c - n_split, plane stride ps1h (planar X2F16 only);
 *                           rows < raw_rows also store acc + bias (fp32) at
 *                           raw[r][c - n_split] (ld_raw); *range_flag |= 1 if a
 *                           GELU value leaves the x2f16 range
 *            TVR_EPI_RESID  out0 = acc + bias + resid[r][c] (ldr)
 *            out0m (bias, GELU): output rows < mirror_rows of the fp32 columns
 *            are also written to out0m (row stride ld0).  bias, range_flag,
 *            raw, out0m may be NULL.
 *   a_rows   host [M] or NULL: launch row r reads row a_rows[r] of A / a2
 *            (a buffer of a_buf_rows rows)
 *   out_rows host [M] or NULL, distinct: launch row r is row out_rows[r] of
 *            out0, out0m, out1h and resid (buffers of out_buf_rows rows)
 *   a2, a2_col  column tiles whose first column is >= a2_col (a multiple of
 *            256) read a2 instead of A
 *   skinny   opt in to the skinny kernel (taken for M <= 16 on two weight
 *            planes, planar layout, bias epilogue, no out_rows / a2)
 *   form     TVR_FORM_PLAN: the engine's own plan for (M, N, K) (plan_pp_cached,
 *            as a block calls it; tvr_gemm_plan reports it); forced forms:
 *            TVR_FORM_PLAIN; TVR_FORM_SPLITK every tile split form_n ways;
 *            TVR_FORM_TAIL tiles [0, form_tile) plain, the rest split form_n
 *            ways; TVR_FORM_STREAMK tiles [0, form_tile) plain, the rest
 *            stream-K over form_n blocks
 *   slicing  the x2f16 sliced accumulation: TVR_SLICE_MODEL the engine's rule
 *            (pp_sliced_rule: K or the model's K2 >= 16384), TVR_SLICE_ON,
 *            TVR_SLICE_OFF
 * All arguments are validated on the host before any device call and before
 * the model is read: TVR_ERR_INVALID for a null model / args / A / W / out0, an
 * unknown fmt, exact16, epi, form, slicing or skinny, M, N or K <= 0, K not a
 * multiple of the k-tile (32; BF16 64), w_scale not positive and finite, lda <
 * K or not a multiple of 8 (32 interleaved), ldw < K or not a multiple of 8,
 * wps too small or not a multiple of 8, ld0 < N, a data buffer that is not
 * 16-byte aligned, an a_rows / out_rows entry outside its buffer or an output
 * row named twice, a2_col not a multiple of 256, the residual epilogue without
 * resid, with ldr < N or with out0m, mirror_rows or raw_rows outside their
 * rows, raw with out_rows, n_split outside [0, N], GELU strides too small for
 * the columns (or, with N and every stride a multiple of 4 — the vector
 * epilogue — ld1h, ps1h, n_split not multiples of 8, ld_raw not of 4), exact16
 * with BF16, exact16 2 with any fmt but TVR_ACT_X2F16_IL (TVR_ERR_UNSUPPORTED
 * on a build without the wide one-plane tile), the interleaved layout with two weight planes and anything but
 * the plain bias launch, skinny with a forced split, a mirror or another
 * epilogue; a forced split or stream-K without the vector epilogue, form_tile
 * outside the raster of 256 x 256 tiles, a split S < 2 or with fewer than 8
 * k-tiles per part or more than 4096 partial tiles, stream-K blocks below the
 * tile count, above 256 or above tiles x k-tiles.  The fused-statistics
 * epilogue is not reachable here.  A test primitive: it copies the row
 * indices to a temporary device buffer and synchronises `stream`.
 * (Backward-compatible addition: ABI 11.) */
enum tvr_gemm_epi { TVR_EPI_BIAS = 0, TVR_EPI_GELU = 1, TVR_EPI_RESID = 2 };
enum tvr_gemm_form { TVR_FORM_PLAN = 0, TVR_FORM_PLAIN = 1, TVR_FORM_SPLITK = 2, TVR_FORM_TAIL = 3,
                     TVR_FORM_STREAMK = 4 };
enum tvr_gemm_slicing { TVR_SLICE_MODEL = 0, TVR_SLICE_ON = 1, TVR_SLICE_OFF = 2 };
typedef struct tvr_gemm_args {
  int32_t fmt, exact16, epi, form, form_n, form_tile, slicing, skinny;
  int32_t M, N, K, lda, ldw, ld0, n_split, ld1h;
  int32_t ps1h, raw_rows, ld_raw, mirror_rows, ldr, a2_col, a_buf_rows, out_buf_rows;
  float w_scale;
  int32_t reserved;
  uint64_t wps;
  const uint16_t* A;
  const uint16_t* a2;
  const uint16_t* W;
  const float* bias;
  float* out0;
  float* out0m;
  uint16_t* out1h;
  float* raw;
  const float* resid;
  uint32_t* range_flag;
  const int32_t* a_rows;
  const int32_t* out_rows;
} tvr_gemm_args;
int tvr_gemm_launch(tvr_model* model, const tvr_gemm_args* args, void* stream);

/* The site entry of the patch sweeps alone, on a caller's rows: the sites are
 * planned exactly as tvr_patch_sweep / tvr_patch_sweep_sets plan them on a
 * filled trace (entry layers, shared prefixes, head groups), every entry layer
 * 0 .. n_layers runs the sweep's own entry launches, and the rows each site
 * materialises (its resid_pre at its entry layer) are left in `out`.  Nothing
 * else of a sweep runs.
 *   seq_lens   host [n_seq], each in [1, n_ctx]: sequence s is the rows
 *              [sum of the lengths before it, + seq_lens[s]) of every layer
 *   token_ids  host [sum seq_lens] or NULL.  Given (and TVR_PREFIX_SHARE not 0):
 *              REPLACE_HEAD sites share prefixes as in the sweep, so a follower
 *              materialises the positions [p0, T) only
 *   tokens     rows per layer of resid and z (>= sum seq_lens)
 *   resid      device [n_layers + 1][tokens][d]: hook_resid_pre, the trace's layout
 *   z          device [n_layers][tokens][d]: attn.hook_z
 *   sites, vectors, n_vectors   as tvr_patch_sweep
 *   set_off, patches            as tvr_patch_sweep_sets, or both NULL: the plain
 *              sweep's planning (a head-set site enters as a copy of its clean rows)
 *   flags      TVR_ENTRY_FORCE_VALU: REPLACE_HEAD sites take entry_kernel's own
 *              VALU branch (the fallback for head sizes without an MFMA entry
 *              kernel) instead of the MFMA kernel
 *   out        device [out_rows][d]: site i's rows are
 *              out[site_row0[i] .. site_row0[i] + site_rows[i]), the positions
 *              [site_p0[i], site_p0[i] + site_rows[i]) of its sequence; rows past
 *              the sum of site_rows are not written
 *   site_row0, site_rows, site_p0   host [n_sites]: the planner's values
 * All arguments are validated on the host before any device call:
 * TVR_ERR_INVALID for a null model / seq_lens / resid / z / sites / out / report
 * array, n_seq <= 0, n_sites <= 0, a length outside [1, n_ctx], a layout that
 * exceeds `tokens`, resid, z or out not 16-byte aligned, unknown flags, set_off
 * or patches as tvr_patch_sweep_sets refuses them, every site the sweeps
 * refuse, more rows than out_rows — and, stricter than tvr_patch_sweep, a
 * REPLACE_HEAD site with `vectors` not 16-byte aligned (its kernels load 16
 * bytes).  A test primitive: it copies the tables to a temporary device buffer
 * and synchronises `stream`.  (Backward-compatible addition: ABI 11.) */
enum { TVR_ENTRY_FORCE_VALU = 1 };
int tvr_site_entry(tvr_model* model, const int32_t* seq_lens, int32_t n_seq, const int32_t* token_ids,
                   int32_t tokens, const float* resid, const float* z, const tvr_site* sites,
                   int32_t n_sites, const int32_t* set_off, const tvr_head_patch* patches,
                   const float* vectors, int32_t n_vectors, int32_t flags, float* out, int32_t out_rows,
                   int32_t* site_row0, int32_t* site_rows, int32_t* site_p0, void* stream);

/* One head-set patch launch (what a layer of tvr_patch_sweep_sets applies between
 * the attention and the O + MLP-out GEMM) on a caller's buffers: for every item,
 * the listed heads' d_head columns of a2 rows [row0, row0 + n_rows) become zero
 * in every plane, and resid rows [row0, row0 + n_rows) += the sum of the listed
 * vectors: s = ((0 + v0) + v1) + .. in list order, then x + s (fp32).
 *   fmt      0: a2 is fp32 [rows][K2], K2 = d_model + d_mlp; TVR_GEMM_X2F16,
 *            TVR_ACT_X2F16_IL, TVR_GEMM_BF16: halves [rows][2 K2] in the format
 *            tvr_act_rows describes (BF16: the first K2 halves of a row)
 *   items    host [n_items]: rows and the range [first_patch, first_patch +
 *            n_patches) of `patches` (an empty range: nothing is zeroed, s = 0)
 *   patches  host [n_patches]: (head, vec)
 *   vectors  device [n_vectors][d], any float alignment (16-byte aligned with
 *            d % 4 == 0 takes the float4 variant, else the element-wise one)
 *   a2, resid  device, 16-byte aligned; resid [rows][d]
 * All arguments are validated on the host before any device call:
 * TVR_ERR_INVALID for a null model / items / vectors / a2 / resid, null patches
 * with n_patches > 0, n_items <= 0, n_patches < 0, rows <= 0, an unknown fmt, a2
 * or resid not 16-byte aligned, vectors not float aligned, an item with
 * n_rows < 1, rows outside [0, rows) or shared with another item, a patch range
 * outside the list, a head outside [0, n_heads), a vec outside [0, n_vectors).
 * A test primitive: it copies the tables to a temporary device buffer and
 * synchronises `stream`.  (Backward-compatible addition: ABI 11.) */
typedef struct tvr_headset_item { int32_t row0, n_rows, first_patch, n_patches; } tvr_headset_item;
typedef struct tvr_headset_patch { int32_t head, vec; } tvr_headset_patch;
int tvr_headset_apply(tvr_model* model, int32_t fmt, const tvr_headset_item* items, int32_t n_items,
                      const tvr_headset_patch* patches, int32_t n_patches, const float* vectors,
                      int32_t n_vectors, void* a2, float* resid, int32_t rows, void* stream);

/* Kernel timing (HIP events recorded on the launch stream around every GEMM
 * launch while enabled).  tvr_profile_read synchronises the recorded events
 * and returns totals since the last enable; used by bench.py for the
 * roofline's achieved TFLOP/s of the dominant kernel. */
typedef struct tvr_kernel_stats {
  /* index = GEMM epilogue: 0 unembed (bias), 1 QKV+MLP-in (split + GELU),
   * 2 O+MLP-out (bias + parallel residual) */
  int64_t gemm_launches[3];
  double gemm_flops[3];   /* algorithmic 2*M*N*K summed over launches */
  double gemm_ms[3];      /* summed launch durations */
  double gemm_bytes[3];   /* minimal operand bytes (A + W + C) summed */
} tvr_kernel_stats;
int tvr_profile_enable(tvr_model* model, int32_t on);
int tvr_profile_read(tvr_model* model, tvr_kernel_stats* out);

/* The HBM-bound kernels, timed the same way (HIP events around each launch
 * while profiling is enabled) with their algorithmic bytes: achieved GB/s =
 * bytes / ms.  Index = enum tvr_hbm_kind. */
enum tvr_hbm_kind {
  TVR_HBM_ENTRY = 0,      /* patch injection at the entry layer (REPLACE_HEAD / ADD / SET_RESID):
                           * clean rows in, patched rows out, z rows + W_O slice per head; and the head-set
                           * patches of tvr_patch_sweep_sets, one launch per patched layer: z slices zeroed +
                           * residual rows read and written + vectors read */
  TVR_HBM_CAPTURE = 1,    /* extraction: sum of hook_z at every prompt's last row -> [d] per layer; and
                           * tvr_trace_capture_resid: rows read x (L + 1) x d x 4 + out read and written; and
                           * tvr_trace_logit_attribution / tvr_head_attribution: the direction pass's rows, and per
                           * layer of the head pass W_O once per chunk of 16 sequences + the z and direction rows;
                           * and tvr_head_directions / the G pass of tvr_trace_source_attribution: per layer W_O once
                           * per chunk of 16 rows + the direction rows once per head + G written */
  TVR_HBM_LNPRE = 2,      /* LayerNormPre rows -> GEMM input format */
  TVR_HBM_ATTENTION = 3,  /* attention: fp32 Q/K/V rows in, z out (activation format [+ fp32 hook_z]); and
                           * tvr_trace_capture_pattern: per layer the Q row + the K rows read, pattern / mass written;
                           * and the knockout launches of tvr_patch_sweep_knockout, one per layer with members: per
                           * listed head the Q slice + the K and V slices of every key + the z slice, the mask words;
                           * and the source kernel of tvr_trace_source_attribution: per layer the Q row, the g row and
                           * the K and V rows read, the source rows / class sums written */
  TVR_HBM_ROW_STATS = 4,  /* softmax target probability / top-k over one logit row per site */
  TVR_HBM_LIN_ENTRY = 5,  /* linearised entry layer of REPLACE_HEAD sites (the vectors' W1 product G and
                           * the K = d_head entry-row GEMM with its combine epilogue): entering rows' outputs
                           * written + their clean rows' outputs read, z slices, W1 W_O planes once */
  TVR_HBM_KINDS = 6
};
typedef struct tvr_hbm_stats {
  int64_t launches[6];
  double ms[6];     /* summed launch durations */
  double bytes[6];  /* algorithmic bytes summed */
} tvr_hbm_stats;
int tvr_profile_read_hbm(tvr_model* model, tvr_hbm_stats* out);

/* The launch plan the engine uses for one planar GEMM of M x N x K
 * (gemm_pingpong_kernel, 256 x 256 tiles; engine.hip plan_pp): out[0] k-split
 * of the whole launch, out[1] first tile of a split tail (0: none), out[2] the
 * tail's split, out[3] first stream-K tile (-1: none), out[4] stream-K blocks.
 * gemm_mode: TVR_GEMM_X2F16 or TVR_GEMM_BF16; flags bit 0 (TVR_PLAN_GELU):
 * the QKV + MLP-in launch (GELU epilogue); bit 1 (TVR_PLAN_MODEL_SLICED): the
 * launch belongs to a model whose O + MLP-out K reaches the sliced-accumulation
 * threshold (6.9B, 12B: every x2f16 GEMM of such a model runs sliced, as does
 * any launch with K >= that threshold; pp_sliced_rule, the one statement of it
 * that launch_gemm and this entry point share); bit 2 (TVR_PLAN_EXACT16): one exact
 * fp16 weight plane (tvr_model_set_exact16: 2 products, cheaper k-tiles).
 * Host-only, no device call (diagnostics, CPU tests).  (ABI 10; flag bits 1
 * and 2 from round 5) */
enum { TVR_PLAN_GELU = 1, TVR_PLAN_MODEL_SLICED = 2, TVR_PLAN_EXACT16 = 4 };
int tvr_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t gemm_mode, int32_t flags, int32_t* out);

/* Bytes of engine workspace currently held by the model (diagnostics);
 * the weight planes of the split / bf16 modes are not included (X3BF16 6 B,
 * X2F16 4 B, BF16 2 B per GEMM weight). */
size_t tvr_workspace_bytes(const tvr_model* model);

#ifdef __cplusplus
}
#endif

#endif /* TVR_H_ */
