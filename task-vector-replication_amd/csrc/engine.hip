// engine.hip — runtime behind include/tvr.h.
//
// Owns the per-model rotary tables and activation workspace, plans batched
// sweeps (the "staircase": sites sorted by entry layer so the active rows of
// layer l are always a prefix of the activation buffer) and enqueues the
// kernels of kernels.hpp / gemm_f32.hpp on the caller's stream.
//
// Reference loops replaced (see include/tvr.h for the per-entry-point map):
// scratch2.py:81-100 (extraction), :114-150 (layer sweeps), :171-197 (CIE),
// :292-314 (FV eval) and scratch.py:106-147 (residual patch sweep).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "tvr.h"
#include "gemm_f32.hpp"
#include "attention_mfma.hpp"
#include "attention_pattern.hpp"
#include "attention_knockout.hpp"
#include "logit_attribution.hpp"
#include "source_attribution.hpp"
#include "gemm_pingpong.hpp"
#include "gemm_skinny.hpp"
#include "gemm_planar.hpp"
#include "gemm_x2f16.hpp"
#include "gemm_x3bf16.hpp"
#include "kernels.hpp"
#include "lin_entry.hpp"
#include "entry_mfma.hpp"
#include "headset_patch.hpp"
#include "sweep_plan.hpp"

using namespace tvr;

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define TVR_HIP(expr)                                                           \
  do {                                                                          \
    hipError_t _e = (expr);                                                     \
    if (_e != hipSuccess)                                                       \
      return fail(TVR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

#define TVR_TRY(expr)        \
  do {                       \
    int _rc = (expr);        \
    if (_rc != TVR_OK) return _rc; \
  } while (0)

constexpr size_t kAlign = 256;
inline size_t align_up(size_t x) { return (x + kAlign - 1) & ~(kAlign - 1); }

// Bump allocator over one device allocation.
struct Carve {
  size_t off = 0;
  template <class T>
  size_t take(size_t count) {
    const size_t at = off;
    off = align_up(off + count * sizeof(T));
    return at;
  }
};

// Pinned host staging for per-call metadata (descriptors, tokens).  Two
// buffers used alternately; an event guards reuse.
struct Staging {
  void* buf[2] = {nullptr, nullptr};
  size_t cap[2] = {0, 0};
  hipEvent_t done[2] = {nullptr, nullptr};
  bool pending[2] = {false, false};
  int next = 0;
};

// A GEMM weight operand: the fp32 matrix and, in a split mode, its planes
// (plane stride wps elements): TVR_GEMM_X3BF16 three bf16 planes in x;
// the planar modes in h: TVR_GEMM_X2F16 two fp16 planes of w * wscale,
// TVR_GEMM_BF16 one bf16 plane.
struct MatW {
  const float* f = nullptr;
  const uint16_t* x = nullptr;
  const uint16_t* h = nullptr;
  size_t wps = 0;
  float wscale = 1.0f;
  bool x16 = false;  // h is ONE plane holding the weights exactly (fp16 values: tvr_model_set_exact16)
  // x16: the same plane row-pair interleaved (w_layout.hpp), or null.  launch_gemm reads it instead of h where the
  // launch's form has the interleaved-weight kernel (one-plane wide tile on interleaved A); every other reader
  // of the plane reads h.
  const uint16_t* hil = nullptr;
  // from row elems / ld on.  (A pair of the interleaved copy is two rows long: an even row's pair starts at the
  // row's own offset.  w_from_row checks the evenness.)
  MatW rows(size_t elems) const {
    return {f ? f + elems : nullptr, x ? x + elems : nullptr, h ? h + elems : nullptr, wps, wscale, x16,
            hil ? hil + elems : nullptr};
  }
};

// Launch plan of a planar GEMM (plan_pp), cached per (M, N, K, format, GELU epilogue, stream-K switch).
using PlanKey = std::tuple<int, int, int, int, int, int>;
struct PpPlan {
  int ksplit = 1;    // whole launch
  int tail_base = 0; // > 0: tiles [0, tail_base) plain, the rest split tail_split ways
  int tail_split = 1;
  int sk_base = -1;  // >= 0: tiles [0, sk_base) plain, the rest stream-K over sk_blocks blocks
  int sk_blocks = 0;
};
// A caller's launch form for one launch_gemm (tvr_gemm_launch, the test primitive): the plan instead of
// plan_pp_cached's, and the sliced accumulation on (1) or off (2) instead of the model's rule (0).  The caller
// has checked the plan against the shape (vector epilogue, S and G in range, the workspace cap).
struct GemmForce {
  bool plan_set = false;
  PpPlan plan;
  int slicing = 0;
};
}  // namespace

struct tvr_model {
  tvr_config cfg{};
  int D1 = 0;  // 3d + d_mlp
  int K2 = 0;  // d + d_mlp
  const float* w_embed = nullptr;
  std::vector<tvr_layer_weights> layers;
  const float* w_unembed_t = nullptr;
  const float* b_unembed = nullptr;
  float* rot_cos = nullptr;
  float* rot_sin = nullptr;
  const float** d_w2s = nullptr;
  // GEMM operands (x planes set by tvr_model_set_gemm)
  int gemm_mode = TVR_GEMM_F32;
  uint16_t* planes = nullptr;
  unsigned* range_flag = nullptr;  // device word: X2F16 input out of range since the last status read
  std::vector<MatW> w1, w2;
  // TVR_GEMM_BF16 only: W1's Q / K rows [0, 2d) as one fp16 plane of
  // wscale * W (the attention-score projections run on fp16 operands: launch_w1)
  std::vector<MatW> w1qk;
  MatW wu;
  char* ws = nullptr;
  size_t ws_bytes = 0;
  float* splitk_ws = nullptr;  // split-K partial products (launch_gemm), grown on demand
  size_t splitk_bytes = 0;
  Staging staging;
  // profiling (tvr_profile_enable): event pairs around GEMM launches (kind =
  // GEMM epilogue index 0-2) and the HBM-bound kernels (kind 3 + tvr_hbm_kind)
  bool prof = false;
  struct ProfRec { hipEvent_t a, b; int epi; double flops, bytes; };
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> prof_pool;
  // Linearised entry layer (lin_entry.hpp), built on the first patch sweep that
  // uses it in a planar mode and dropped on a mode change: for layers
  // l = 1 .. L-2, Wsc = W1[l] W_O[l-1] as weight planes [NPL][H][D1][KP]
  // (head-major, d_head zero-padded to KP) and c1[l] = row sums of W1[l].
  int lin_mode = -1;
  int lin_failed_mode = -1;  // the planes did not fit in this GEMM mode: the sweeps use the full entry GEMM
  int lin_kp = 0;
  uint16_t* lin_planes = nullptr;  // layer l at (l - 1) * NPL * H * D1 * KP halves
  float* lin_c1 = nullptr;         // [L][D1]
  std::vector<float> lin_scale;    // per layer: X2F16 plane scale (1 for BF16)
  std::map<PlanKey, PpPlan> plans;  // plan_pp_cached: GEMM launch plans per shape
  // Exact-fp16 weights (tvr_model_set_exact16; x2f16 mode only): the checkpoint's own W1 rows (Q | K | V |
  // MLP-in, before fold_ln) and W2 (W_O | W_out, before center_writing_weights) as one caller-owned fp16
  // plane each, and LN1 / LN2's gamma.  The QKV + MLP-in GEMM then reads LNPre(x) * gamma1 (Q, K, V
  // columns) / * gamma2 (MLP-in columns) against the raw rows — fold_ln's centring of the read-in weights
  // is a no-op on a centred LNPre row — and the O + MLP-out GEMM the raw W2, whose missing centring adds one
  // constant to every element of a row's residual, which every LayerNorm (and the centred trace export)
  // removes.  Both then run 2 MFMA products per slice instead of 3 (gemm_pingpong.hpp WX).
  bool x16 = false;
  // the exact-fp16 sweeps' GEMM inputs (xn, xn2, a2, xf) in the k-tile-interleaved layout (ACT_X2F16I, split.hpp);
  // false (TVR_ACT_LAYOUT=planar, read when the GEMM mode is set): the planar [rows][2][K] layout
  bool act_il = true;
  std::vector<MatW> w1x, w2x;
  std::vector<const float*> g1, g2;
  // the unembed's raw W_U [V][d] (one fp16 plane) and the final LN's gamma (tvr_model_set_exact16_unembed): the
  // fused-statistics unembed reads LNPre(x) * gf against it (2 products).  fold_ln's centring is a no-op again,
  // and center_unembed's mean over the vocabulary is one constant per row of logits, which the statistics
  // (softmax probability, top-k) do not see; the logits paths keep the processed W_U.
  MatW wux;
  const float* gf = nullptr;
  // Engine-owned row-pair-interleaved copies (w_layout.hpp) of the bound raw planes, which the one-plane GEMMs on
  // interleaved activations stage as whole 128-B lines: every layer's W1 and W2 in one allocation, W_U in its own
  // (+2 B per parameter; the caller's planes stay bound).  Built by sync_w_il whenever the exact-fp16 path is on
  // in the interleaved activation layout, dropped when it goes off or the binding changes.  w_il_wanted: false
  // under TVR_W_LAYOUT=rows (read when the layers are bound).  w_il_nomem: a copy did not fit; the model runs on
  // the plain planes (tvr_model_weight_layout reports it).
  uint16_t* w_il = nullptr;
  uint16_t* wu_il = nullptr;
  bool w_il_wanted = true;
  bool w_il_nomem = false;
};

struct tvr_trace {
  tvr_model* model = nullptr;
  int max_seqs = 0, max_tokens = 0;
  float* resid = nullptr;  // [L+1][max_tokens][d]
  float* z = nullptr;      // [L][max_tokens][d]
  float* qkv = nullptr;    // [L][max_tokens][3d]
  std::vector<int> seq_off, seq_len;
  std::vector<int32_t> tokens;  // host copy of the traced ids (shared-prefix detection in patch sweeps)
  int n_seq = 0, n_tokens = 0;
  // A deferred clean forward (tvr_forward_clean_deferred): the metadata above
  // is set, the buffers are not; the next tvr_patch_sweep on this trace runs
  // the clean rows inside its own launches (filling the buffers as
  // tvr_forward_clean would) and writes these outputs; any other use of the
  // trace runs it on its own first (flush_pending).
  bool pending = false;
  bool uncentred = false;  // filled on the exact-fp16 weight path: hook_resid_pre is centred on export
  std::vector<int32_t> p_targets;  // [n_seq] or empty
  float* p_prob = nullptr;
  int32_t* p_topk = nullptr;
  int p_k = 0;
  void* p_stream = nullptr;  // the stream of the deferral (its inputs / outputs are ordered on it)
};

namespace {

constexpr int kFinalChunk = 1024;

int ensure_workspace(tvr_model* m, size_t bytes, hipStream_t st) {
  if (bytes <= m->ws_bytes) return TVR_OK;
  TVR_HIP(hipStreamSynchronize(st));
  if (m->ws) TVR_HIP(hipFree(m->ws));
  m->ws = nullptr;
  m->ws_bytes = 0;
  const size_t want = align_up(bytes + bytes / 8);
  if (hipMalloc(&m->ws, want) != hipSuccess) {
    m->ws = nullptr;
    (void)hipGetLastError();
    return fail(TVR_ERR_NOMEM, "workspace allocation of " + std::to_string(want) + " bytes failed");
  }
  m->ws_bytes = want;
  return TVR_OK;
}

int ensure_splitk(tvr_model* m, size_t bytes, hipStream_t st) {
  if (bytes <= m->splitk_bytes) return TVR_OK;
  TVR_HIP(hipStreamSynchronize(st));
  if (m->splitk_ws) TVR_HIP(hipFree(m->splitk_ws));
  m->splitk_ws = nullptr;
  m->splitk_bytes = 0;
  const size_t want = align_up(bytes);
  if (hipMalloc(&m->splitk_ws, want) != hipSuccess) {
    m->splitk_ws = nullptr;
    (void)hipGetLastError();
    return fail(TVR_ERR_NOMEM, "split-K workspace allocation of " + std::to_string(want) + " bytes failed");
  }
  m->splitk_bytes = want;
  return TVR_OK;
}

// Copy host bytes to device through pinned staging (async on `st`).
int upload(tvr_model* m, hipStream_t st, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return TVR_OK;
  Staging& s = m->staging;
  const int i = s.next;
  s.next ^= 1;
  if (s.pending[i]) {
    TVR_HIP(hipEventSynchronize(s.done[i]));
    s.pending[i] = false;
  }
  if (s.cap[i] < bytes) {
    if (s.buf[i]) TVR_HIP(hipHostFree(s.buf[i]));
    s.buf[i] = nullptr;
    const size_t want = align_up(std::max(bytes, (size_t)1 << 20));
    TVR_HIP(hipHostMalloc(&s.buf[i], want, hipHostMallocDefault));
    s.cap[i] = want;
  }
  if (!s.done[i]) TVR_HIP(hipEventCreateWithFlags(&s.done[i], hipEventDisableTiming));
  std::memcpy(s.buf[i], src, bytes);
  TVR_HIP(hipMemcpyAsync(dst, s.buf[i], bytes, hipMemcpyHostToDevice, st));
  TVR_HIP(hipEventRecord(s.done[i], st));
  s.pending[i] = true;
  return TVR_OK;
}

// Several host arrays packed into ONE upload (one staging buffer, one copy).
struct UploadBatch {
  std::vector<char> host;
  struct Item { size_t host_off; size_t dev_off; size_t bytes; };
  std::vector<Item> items;
  template <class T>
  void add(size_t dev_off, const std::vector<T>& v) {
    items.push_back({host.size(), dev_off, v.size() * sizeof(T)});
    const char* p = reinterpret_cast<const char*>(v.data());
    host.insert(host.end(), p, p + v.size() * sizeof(T));
  }
};

int flush_uploads(tvr_model* m, hipStream_t st, char* base, const UploadBatch& ub) {
  // Items are carved contiguously in order, so the batch is one span.
  if (ub.items.empty()) return TVR_OK;
  const size_t first = ub.items.front().dev_off;
  std::vector<char> span;
  size_t end = first;
  for (const auto& it : ub.items) end = std::max(end, it.dev_off + it.bytes);
  span.assign(end - first, 0);
  for (const auto& it : ub.items)
    std::memcpy(span.data() + (it.dev_off - first), ub.host.data() + it.host_off, it.bytes);
  return upload(m, st, base + first, span.data(), span.size());
}

hipEvent_t prof_event(tvr_model* m) {
  hipEvent_t e = nullptr;
  if (!m->prof_pool.empty()) {
    e = m->prof_pool.back();
    m->prof_pool.pop_back();
  } else if (hipEventCreate(&e) != hipSuccess) {
    e = nullptr;
  }
  return e;
}

// HIP events around one HBM-bound launch (or a short launch sequence) while
// profiling: done(kind, algorithmic bytes) records the closing event.
struct ProfSpan {
  tvr_model* m;
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  ProfSpan(tvr_model* m_, hipStream_t s) : m(m_), st(s) {
    if (m && m->prof) {
      a = prof_event(m);
      b = prof_event(m);
      if (a) (void)hipEventRecord(a, st);
    }
  }
  void done(int kind, double bytes) {
    if (!a || !b) return;
    (void)hipEventRecord(b, st);
    m->prof_recs.push_back({a, b, 3 + kind, 0.0, bytes});
    a = b = nullptr;
  }
  ~ProfSpan() {  // not done (error path): events back to the pool
    if (a) m->prof_pool.push_back(a);
    if (b) m->prof_pool.push_back(b);
  }
};

// TVR_PREFIX_SHARE=0 turns off shared-prefix rows in tvr_forward_clean /
// tvr_patch_sweep (read per call; the tests run both settings and compare).
bool env_flag(const char* name) {
  const char* e = getenv(name);
  return !(e && std::string(e) == "0");
}
bool prefix_share_enabled() { return env_flag("TVR_PREFIX_SHARE"); }
// TVR_LIN_ENTRY=0 runs the entry layer of REPLACE_HEAD sites through the full
// GEMM instead of lin_entry.hpp (the tests compare both).
bool lin_entry_enabled() { return env_flag("TVR_LIN_ENTRY"); }

// Activation format of the model's GEMM inputs (split.hpp).
int act_fmt(const tvr_model* m) {
  return m->gemm_mode == TVR_GEMM_X2F16 ? ACT_X2F16 : m->gemm_mode == TVR_GEMM_BF16 ? ACT_BF16 : ACT_F32;
}

// the exact-fp16 weight path (tvr_model_set_exact16) is on: x2f16 mode with the raw planes attached
bool use_x16(const tvr_model* m) { return m->x16 && m->gemm_mode == TVR_GEMM_X2F16; }

// TVR_ACT_LAYOUT=planar keeps the exact-fp16 sweeps' GEMM inputs in the planar layout (A/B runs, tests)
bool act_layout_interleaved() {
  const char* e = getenv("TVR_ACT_LAYOUT");
  return !(e && std::string(e) == "planar");
}
// TVR_W_LAYOUT=rows keeps the exact-fp16 GEMMs on the caller's plain planes: no interleaved copies (A/B runs,
// tests, fallback)
bool w_layout_interleaved() {
  const char* e = getenv("TVR_W_LAYOUT");
  return !(e && std::string(e) == "rows");
}
// Format of the sweep buffers xn, xn2, a2 and xf (Acts::fmt): on the exact-fp16 path the interleaved layout,
// which only the one-plane GEMM reads; the side buffers (vact, vg, G) keep act_fmt's planar layout.
int acts_fmt(const tvr_model* m) { return use_x16(m) && m->act_il ? (int)ACT_X2F16I : act_fmt(m); }

// Raster group (m-blocks walked before the next block column): 4, or 2 when
// there are at most 16 block columns (tools/gemm_split_probe x2ppgm<N>: at
// M = 90,000 the qkv shape ran 459 / 451 / 419 TF at 4 / 8 / 16, the
// MLP-out shape (10 columns) 470 / 466 / 458 at 2 / 4 / 8).
// A/B knobs TVR_PP_GM_SMALL / TVR_PP_GM_LARGE (read once) override the two values.
int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e && *e ? atoi(e) : dflt;
}
int pp_group_m(int N) {
  static const int small = env_int("TVR_PP_GM_SMALL", 2), large = env_int("TVR_PP_GM_LARGE", 4);
  return (N + 255) / 256 <= 16 ? small : large;
}

// gemm_pingpong_kernel `kp` (pp_kernel of the launch's form) over tiles [tile_base, tile_base + count) of a
// planar launch's raster (count 0: all)
void launch_pp(PpKernel kp, const uint16_t* Ah, int lda, const MatW& W, int ldw, int M, int N, int K,
               const GemmEpi& ep0, float acc_scale, int tile_base, int count, hipStream_t st) {
  GemmEpi ep = ep0;
  ep.tile_base = tile_base;
  ep.tile_count = count;
  ep.group_m = pp_group_m(N);
  const dim3 g(count > 0 ? count : gemm_pingpong_grid(M, N));
  hipLaunchKernelGGL(kp, g, dim3(PP_THREADS), 0, st, Ah, 2 * lda, (size_t)lda, W.h, ldw, W.wps, acc_scale, M, N, K, ep);
}

// One planned planar GEMM, resolved before anything is launched (resolve_pp): tiles [0, base) by `whole`, and
// with n > 0 the tiles from `base` on as fp32 partial tiles, split-K n ways or stream-K over n blocks.
struct PpLaunch {
  PpKernel whole = nullptr;              // the launch's own epilogue (n == 0: every tile)
  PpKernel partial = nullptr;            // EPI_BIAS, VEC partial tiles
  PpReduceKernel reduce = nullptr;       // after split-K partials
  PpSkReduceKernel sk_reduce = nullptr;  // after stream-K partials
  bool skm = false;
  int base = 0, n = 0;
};

// The partial range of `pl`: tiles [base, base + count) as fp32 partial tiles in the model's split-K workspace,
// then the reduce kernel, which sums each tile's partials in k order and applies the epilogue (deterministic).
// Split-K: K split over n blocks per tile (splitk_reduce_kernel).  Stream-K: n blocks share the range's
// k-iterations evenly (gemm_pingpong_kernel sk_blocks; splitk_sk_reduce_kernel).
int launch_pp_partial(const PpLaunch& pl, const uint16_t* Ah, int lda, int a_fmt, const MatW& W, int ldw, int M, int N,
                      int K, const GemmEpi& ep0, float acc_scale, int count, tvr_model* m, hipStream_t st) {
  const int n = pl.n;
  const size_t ws_tiles = pl.skm ? (size_t)2 * n : (size_t)n * count;
  const int rc = ensure_splitk(m, ws_tiles * PP_TILE_ELEMS * sizeof(float), st);
  if (rc != TVR_OK) return rc;
  GemmEpi ep = ep0;  // the reduce's epilogue: same raster as the partial launch
  ep.group_m = pp_group_m(N);
  GemmEpi pe{};
  pe.group_m = ep.group_m;
  pe.out0 = m->splitk_ws;
  pe.a_rows = ep.a_rows;
  if (pl.skm) pe.sk_blocks = n; else pe.k_split = n;
  pe.tile_base = pl.base;
  pe.tile_count = count;
  pe.a2 = ep.a2;  // the exact-fp16 QKV + MLP-in launch's second A operand (by column)
  pe.a2_col = ep.a2_col;
  const dim3 g(pl.skm ? n : count * n);
  const dim3 rg((unsigned)std::min<long>(4096, ((long)count * (PP_TILE_ELEMS / 4) + 255) / 256));
  hipLaunchKernelGGL(pl.partial, g, dim3(PP_THREADS), 0, st, Ah, 2 * lda, (size_t)lda, W.h, ldw, W.wps, acc_scale, M,
                     N, K, pe);
  const float* part = (const float*)m->splitk_ws;
  if (pl.skm)
    hipLaunchKernelGGL(pl.sk_reduce, rg, dim3(256), 0, st, part, n, K / pp_ktile(a_fmt), pl.base, count, M, N, ep);
  else
    hipLaunchKernelGGL(pl.reduce, rg, dim3(256), 0, st, part, n, pl.base, count, M, N, ep);
  return TVR_OK;
}

// Launch shape of a planar GEMM on 256 CUs (gemm_pingpong_kernel, one block
// per CU): the whole launch plain, the whole launch split over K (fp32
// partials + splitk_reduce_kernel), or its last tiles split (a partly empty
// last round), and — opt-in, TVR_STREAM_K=1 — stream-K for the last round.
// Launches of up to 1,024 tiles (the small-M layer sweeps: C2's M = 156 + 52 l
// rows) are planned by simulating the dispatch (plan_sim): blocks in
// blockIdx order through the kernel's XCD remap onto the first free of 256
// CUs, a block costing its k-tiles at a rate set by its tile's real rows (a
// wave group skips the MFMAs of its padding 16-row slices; the staging
// remains) plus prologue and epilogue, a split plan the reduce's partial round
// trip on top.  Larger launches keep the round heuristic (their full rounds
// dominate).  Costs in us: profiles/r03/c2_sweep_dispatches_r03f.txt (a C2
// sweep per dispatch: 1.5-2.2 us per x2f16 k-tile per block, reduce at ~5 TB/s).
// stream-K is opt-in: on the C2 sweeps it measured slower than the split-K
// plan (O + MLP-out 8.2 vs 5.7 ms per sweep) and equal on C3
// (profiles/r03/c2_stream_k_ab.txt)
// TVR_STREAM_K: "1" every planned launch, "O" the O + MLP-out launches only (EPI_RESID: 10 column tiles at
// 2.8B, so a rank's share of a split sweep ends in partly filled rounds), else off
int sk_mode() {
  const char* e = getenv("TVR_STREAM_K");
  return !e ? 0 : std::string(e) == "1" ? 1 : std::string(e) == "O" ? 2 : 0;
}
bool sk_enabled(int epi = EPI_BIAS) {
  const int md = sk_mode();
  return md == 1 || (md == 2 && epi == EPI_RESID);
}

struct PlanCost {
  double kt_us, pro_us, epi_us, part_us;
};

// Simulated time (us) of tiles [t0, t0 + cnt) of the raster launched with S
// blocks per tile (S = 1: plain epilogue; S > 1: partial tiles, no reduce).
double plan_sim(int M, int N, int nkt, int t0, int cnt, int S, const PlanCost& pc) {
  const int nbm = (M + 255) / 256, nbn = (N + 255) / 256, gm = pp_group_m(N);
  const int nb = cnt * S, P = 256;
  std::vector<double> cu(P, 0.0);  // CU free times (a min-heap)
  auto remap = [](int bid, int nwg) {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  };
  double end = 0.0;
  for (int b = 0; b < nb; ++b) {
    const int wgs = remap(b, nb), lt = wgs / S, split = wgs - lt * S;
    int m0, n0;
    pp_tile_coords(t0 + lt, nbm, nbn, m0, n0, gm);
    (void)n0;
    const int rows = std::min(256, M - m0);
    const int s0 = (std::min(rows, 128) + 15) / 16, s1 = (std::max(rows - 128, 0) + 15) / 16;
    const double frac = 0.3 + 0.7 * std::max(s0, s1) / 8.0;
    const int kb = (int)((long long)split * nkt / S), ke = (int)((long long)(split + 1) * nkt / S);
    const double dur = pc.pro_us + (ke - kb) * pc.kt_us * frac + (S > 1 ? pc.part_us : pc.epi_us);
    std::pop_heap(cu.begin(), cu.end(), std::greater<double>());
    cu.back() += dur;
    end = std::max(end, cu.back());
    std::push_heap(cu.begin(), cu.end(), std::greater<double>());
  }
  return end;
}

// the split-K reduce of tiles [t0, t0 + cnt) over S partials: launch + partials read + output written
double plan_reduce_us(int M, int N, int t0, int cnt, int S) {
  const int nbm = (M + 255) / 256, nbn = (N + 255) / 256, gm = pp_group_m(N);
  double rows = 0.0;
  for (int t = t0; t < t0 + cnt; ++t) {
    int m0, n0;
    pp_tile_coords(t, nbm, nbn, m0, n0, gm);
    rows += std::min(256, M - m0) * (double)std::min(256, N - n0);
  }
  return 4.0 + rows * 4.0 * (2.0 * S + 1.0) / 5.0e6;  // partials written (by the GEMM) + read, output written
}

// sliced: the launch runs the x2f16 sliced accumulation (~13 % more per k-tile: gemm_pingpong.hpp); wx: one
// exact weight plane, 2 products (0.72 of the 3-product k-tile, 0.85 sliced: profiles/r05/wx_probe_r05r.jsonl)
PpPlan plan_pp(int M, int N, int K, int a_fmt, int epi, bool sliced = false, bool wx = false) {
  PpPlan p;
  const int tiles = gemm_pingpong_grid(M, N), nkt = K / pp_ktile(a_fmt);
  const double kt_scale = wx ? (sliced ? 0.85 : 0.72) : 1.0;
  const double kt_us = (a_fmt == ACT_X2F16 ? 1.9 : 1.3) * (sliced ? 1.13 : 1.0) * kt_scale, seg_us = 15.0,
               epi_us = 10.0;
  // stream-K of `cnt` tiles over min(256, iterations) blocks vs one plain round
  auto sk_us = [&](int cnt) {
    const int G = (int)std::min<long long>(256, (long long)cnt * nkt);
    return std::ceil((double)cnt * nkt / G) * kt_us + 2.0 * seg_us + (cnt + 2.0 * G) * 0.0655 + 5.0;
  };
  const double round_plain_us = nkt * kt_us + epi_us;
  if (sk_enabled(epi) && (long long)tiles * nkt >= 4LL * 256) {
    const int rounds = (tiles + 255) / 256;
    const int tb = tiles - 256 * (rounds - 1);  // tiles of the last (partly empty) round
    if (tb < 256 && sk_us(tb) + 5.0 < round_plain_us) {
      p.sk_base = tiles - tb;
      p.sk_blocks = (int)std::min<long long>(256, (long long)tb * nkt);
      return p;
    }
  }
  if (tiles <= 1024) {
    const PlanCost pc{kt_us, 3.0, epi == EPI_SPLIT_GELU_ACT ? 15.0 : 10.0, 7.0};
    double best = plan_sim(M, N, nkt, 0, tiles, 1, pc);
    // at most 4,096 partial tiles (1 GiB of split-K workspace, which only grows: ensure_splitk)
    for (int S = 2; S <= 16 && nkt / S >= 8 && tiles * S <= 4096; ++S) {
      const double c = plan_sim(M, N, nkt, 0, tiles, S, pc) + plan_reduce_us(M, N, 0, tiles, S);
      if (c < best * 0.97) {  // a split must win clearly: the model is approximate
        best = c;
        p.ksplit = S;
      }
    }
    if (tiles > 256) {
      const int base = 256 * ((tiles - 1) / 256), cnt = tiles - base;
      const double head = plan_sim(M, N, nkt, 0, base, 1, pc);
      for (int S = 2; S <= 16 && nkt / S >= 8; ++S) {
        const double c = head + plan_sim(M, N, nkt, base, cnt, S, pc) + plan_reduce_us(M, N, base, cnt, S);
        if (c < best * 0.97) {
          best = c;
          p.ksplit = 1;
          p.tail_base = base;
          p.tail_split = S;
        }
      }
    }
    return p;
  }
  const int rounds = (tiles + 255) / 256;
  const int tb = tiles - 256 * (rounds - 1);
  if (tb > 224) return p;
  int best = 1;
  double br = 1.0;
  for (int s = 2; s <= 16 && nkt / s >= 8; ++s) {
    const double r = std::ceil(tb * (double)s / 256.0) / s;
    if (r < br - 1e-9) {
      br = r;
      best = s;
    }
  }
  if (best < 2) return p;
  const double round_us = nkt * 2.5 * kt_scale;  // ~2.3-2.7 us per k-tile per block (profiles/gemm_pingpong_anatomy_r01.jsonl)
  const double saved_us = (1.0 - br) * round_us;
  const double cost_us = (best + 1.0) * tb * (double)PP_TILE_ELEMS * 8.0 / 5.0e6;  // partials written + read, ~5 TB/s
  if (saved_us > 1.5 * cost_us + 10.0) {
    p.tail_base = 256 * (rounds - 1);
    p.tail_split = best;
  }
  return p;
}

// plan_pp, cached per launch shape on the model (the sweeps repeat their
// per-layer shapes: the simulation runs once per shape)
PpPlan plan_pp_cached(tvr_model* m, int M, int N, int K, int a_fmt, int epi, bool wx = false) {
  const PlanKey key{M, N, K, a_fmt + (wx ? 16 : 0), epi == EPI_SPLIT_GELU_ACT ? 1 : epi == EPI_RESID ? 2 : 0, sk_mode()};
  auto it = m->plans.find(key);
  if (it != m->plans.end()) return it->second;
  const PpPlan p = plan_pp(M, N, K, a_fmt, epi, a_fmt == ACT_X2F16 && pp_sliced_rule(K, m->K2), wx);
  if (m->plans.size() > 4096) m->plans.clear();
  m->plans.emplace(key, p);
  return p;
}

// The kernels and ranges of `plan` for a planar GEMM whose whole-epilogue form is `f`.  A form without an
// instantiation is an engine error, not another form's launch (launch_gemm's argument checks keep every caller's
// arguments off such a form).
int resolve_pp(const PpForm& f, const PpPlan& plan, PpLaunch& pl) {
  auto missing = [](const char* what, const PpForm& g) {
    return fail(TVR_ERR_INTERNAL, std::string("gemm: no ") + what + " is instantiated for the form epi " +
                                      std::to_string(g.epi) + ", fmt " + std::to_string(g.fmt) + ", vec " +
                                      std::to_string(g.vec) + ", stream-K " + std::to_string(g.skm) + ", sliced " +
                                      std::to_string(g.sl) + ", one weight plane " + std::to_string(g.wx) +
                                      ", interleaved A " + std::to_string(g.ail) + ", interleaved W " +
                                      std::to_string(g.wil));
  };
  pl.skm = plan.sk_base >= 0;
  const bool whole_split = !pl.skm && plan.ksplit > 1, tail_split = !pl.skm && !whole_split && plan.tail_base > 0;
  pl.base = pl.skm ? plan.sk_base : tail_split ? plan.tail_base : 0;
  pl.n = pl.skm ? plan.sk_blocks : whole_split ? plan.ksplit : tail_split ? plan.tail_split : 0;
  if (pl.n == 0 || pl.base > 0) {
    PpForm whole = f;
    whole.vec = f.vec || pl.n > 0;  // the tiles ahead of a partial range run the vector epilogue (a plan needs it)
    pl.whole = pp_kernel(whole);
    if (!pl.whole) return missing("gemm_pingpong_kernel", whole);
  }
  if (pl.n > 0) {
    PpForm part = f;  // fp32 partial tiles
    part.epi = EPI_BIAS;
    part.vec = true;
    part.skm = pl.skm;
    pl.partial = pp_kernel(part);
    if (!pl.partial) return missing("partial-tile gemm_pingpong_kernel", part);
    const int out_fmt = pp_reduce_fmt(f.fmt, f.ail);
    if (pl.skm)
      pl.sk_reduce = pp_reduce_kernel<true>(f.epi, out_fmt);
    else
      pl.reduce = pp_reduce_kernel<false>(f.epi, out_fmt);
    if (!pl.sk_reduce && !pl.reduce) return missing("reduce kernel", part);
  }
  return TVR_OK;
}

// C = A @ W^T with epilogue `epi`.  A is fp32 [M][lda] (a_fmt ACT_F32:
// gemm_f32_nt_kernel, or the in-GEMM splits of the primitive ABI entry points
// when W carries x3bf16 / x2f16 planes) or a planar activation format
// (split.hpp: lda logical elements per row) with the same format's weight
// planes (W.h): gemm_pingpong_kernel, split-K below 192 tiles and a split last
// round when it pays (plan_pp; not for EPI_STATS, whose statistics exist only
// in the whole-K LDS epilogue).
int launch_gemm(int epi, const void* A, int lda, int a_fmt, const MatW& W, int ldw, int M, int N,
                int K, const GemmEpi& ep, hipStream_t st, tvr_model* m = nullptr,
                unsigned* range_flag = nullptr, const GemmForce* force = nullptr) {
  if (M <= 0 || N <= 0) return TVR_OK;
  // ACT_X2F16I: x2f16 values, A's addresses interleaved (ail); the kernels' FMT stays ACT_X2F16.  The one-plane
  // GEMM takes every epilogue and plan, two weight planes the plain EPI_BIAS launch only (no model, no plan).
  const bool ail = a_fmt == ACT_X2F16I;
  if (ail) {
    a_fmt = ACT_X2F16;
    if (!W.x16 && (epi != EPI_BIAS || m || ep.skinny))
      return fail(TVR_ERR_INVALID, "gemm: the interleaved activation layout belongs to the one-plane exact-fp16 GEMMs");
  }
  const bool planar = a_fmt != ACT_F32;
  if (planar && !W.h) return fail(TVR_ERR_INVALID, "gemm: planar activations need the planar weight planes");
  if (epi == EPI_SPLIT_GELU_ACT && !planar)
    return fail(TVR_ERR_INVALID, "gemm: the activation-format GELU epilogue belongs to the planar paths");
  if (epi == EPI_SPLIT_GELU && planar)
    return fail(TVR_ERR_INVALID, "gemm: planar paths write GELU columns in their activation format");
  if (epi == EPI_STATS && (!planar || N % 4 != 0 || !ep.stats))
    return fail(TVR_ERR_INVALID, "gemm: the fused statistics epilogue needs a planar format, N % 4 == 0 and a "
                                 "statistics buffer");
  if (a_fmt == ACT_F16 && epi != EPI_BIAS)
    return fail(TVR_ERR_INVALID, "gemm: the fp16 operand format has the plain (bias) epilogue only");
  if (W.x16 && a_fmt != ACT_X2F16)
    return fail(TVR_ERR_INVALID, "gemm: one-plane exact fp16 weights take x2f16 activations");
  if (ep.a2 && (a_fmt == ACT_F32 || ep.a2_col % 256 != 0))
    return fail(TVR_ERR_INVALID, "gemm: a second A operand needs a planar format and a 256-column boundary");
  if (K % GEMM_BK != 0 || lda % 4 != 0 || ldw % 4 != 0 || ((W.x || W.h) && ldw % 8 != 0) ||
      ((a_fmt == ACT_BF16 || a_fmt == ACT_F16) && K % 64 != 0))
    return fail(TVR_ERR_UNSUPPORTED, "gemm: K, lda, ldw must be multiples of 32/4/4 (8 for planes, K of 64 for "
                                     "bf16; K=" + std::to_string(K) + ")");
  // the planar launch's form, plan and kernels, before any event or launch
  const bool wx = a_fmt == ACT_X2F16 && W.x16;  // one exact fp16 weight plane: 2 products per k-step
  // the plane's row-pair-interleaved copy, where there is one and the launch's form has the kernel for it (the
  // wide one-plane tile on interleaved A); planar A, the narrow-tile build and the skinny kernel read W.h
  const bool wil = wx && ail && W.hil != nullptr && pp_wil_available();
  MatW Wl = W;  // the weight operand as the planar kernels read it
  if (wil) Wl.h = W.hil;
  bool vec = false, sl = false, skinny = false;
  PpLaunch pl;
  if (planar) {
    vec = planar_epilogue_vec(epi, ep, N);
    // x2f16 sliced accumulation (gemm_pingpong.hpp) on every GEMM of a model whose O + MLP-out K reaches
    // PP_SLICE_MIN_K (6.9B, 12B), or on any launch of that K
    // (one-plane weights, A/B of the precision it costs: TVR_WX_SLICE=0 runs them unsliced, 2 slices the
    // O + MLP-out launches only)
    static const int wx_slice = env_int("TVR_WX_SLICE", 1);
    sl = force && force->slicing ? a_fmt == ACT_X2F16 && force->slicing == 1
                                 : a_fmt == ACT_X2F16 && pp_sliced_rule(K, m ? m->K2 : 0) &&
                                       (!wx || wx_slice == 1 || (wx_slice == 2 && epi == EPI_RESID));
    // a few rows (the linearised entry's G on a rank of a head split): gemm_skinny.hpp
    skinny = ep.skinny && epi == EPI_BIAS && M <= SK_USE_M && !ep.out_rows && ep.k_split <= 1 && vec &&
             a_fmt != ACT_F16 && !wx && !ep.a2 && !ail;
    if (!skinny) {
      PpPlan plan;
      if (force && force->plan_set)
        plan = force->plan;
      else if (m && vec && epi != EPI_STATS)
        plan = plan_pp_cached(m, M, N, K, a_fmt, epi, wx);
      // EPI_STATS has the LDS (vector) epilogue only, whatever planar_epilogue_vec said (N % 4 == 0: above)
      TVR_TRY(resolve_pp(PpForm{epi, a_fmt, vec || epi == EPI_STATS, false, sl, wx, ail, wil}, plan, pl));
    }
  }
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (m && m->prof) {
    ev0 = prof_event(m);
    ev1 = prof_event(m);
    if (ev0) TVR_HIP(hipEventRecord(ev0, st));
  }
  // X2F16: both operands scaled (W by wscale, A by 16); F16: W only; BF16: neither
  const float acc_scale = a_fmt == ACT_BF16 ? 1.0f : a_fmt == ACT_F16 ? 1.0f / W.wscale : 1.0f / (W.wscale * X2_ASCALE);
  if (planar) {
    const uint16_t* Ah = static_cast<const uint16_t*>(A);
    if (skinny) {
      const dim3 g(gemm_skinny_grid(N));
#define TVR_SK(F, MT)                                                                                  \
  hipLaunchKernelGGL((gemm_skinny_kernel<F, MT>), g, dim3(SK_THREADS), 0, st, Ah, 2 * lda, (size_t)lda, W.h, \
                     ldw, W.wps, acc_scale, M, N, K, ep)
#define TVR_SK_F(F)                     \
  switch ((M + 15) / 16) {              \
    case 1: TVR_SK(F, 1); break;        \
    case 2: TVR_SK(F, 2); break;        \
    case 3: TVR_SK(F, 3); break;        \
    default: TVR_SK(F, 4); break;       \
  }
      if (a_fmt == ACT_X2F16) { TVR_SK_F(ACT_X2F16); } else { TVR_SK_F(ACT_BF16); }
#undef TVR_SK_F
#undef TVR_SK
    } else {
      if (pl.n == 0 || pl.base > 0) launch_pp(pl.whole, Ah, lda, Wl, ldw, M, N, K, ep, acc_scale, 0, pl.base, st);
      if (pl.n > 0)
        TVR_TRY(launch_pp_partial(pl, Ah, lda, a_fmt, Wl, ldw, M, N, K, ep, acc_scale,
                                  gemm_pingpong_grid(M, N) - pl.base, m, st));
    }
  } else {
    const float* Af = static_cast<const float*>(A);
    unsigned* flag = m ? m->range_flag : range_flag;
    // exact-product fp32 GEMMs of a model whose O + MLP-out K reaches PP_SLICE_MIN_K (6.9B, 12B), or any launch
    // of that K: the sliced accumulation (gemm_f32.hpp SLICE_KT; the small tile holds the second accumulator set)
    const bool f32_sliced = !W.h && !W.x && pp_sliced_rule(K, m ? m->K2 : 0);
    const bool large = gemm_use_large(M, N) && !f32_sliced;
#define TVR_GEMM_LAUNCH(E, TL)                                                                                    \
  do {                                                                                                            \
    if (f32_sliced)                                                                                               \
      hipLaunchKernelGGL((gemm_f32_nt_kernel<E, TileSmall, F32_SLICE_KT>), dim3(gemm_grid<TileSmall>(M, N)),      \
                         dim3(TileSmall::THREADS), 0, st, Af, lda, W.f, ldw, M, N, K, ep);                        \
    else                                                                                                          \
      hipLaunchKernelGGL((gemm_f32_nt_kernel<E, TL>), dim3(gemm_grid<TL>(M, N)), dim3(TL::THREADS), 0,             \
                         st, Af, lda, W.f, ldw, M, N, K, ep);                                                     \
  } while (0)
#define TVR_X3_LAUNCH(E, TL)                                                                      \
  hipLaunchKernelGGL((gemm_x3bf16_nt_kernel<E, TL>), dim3(gemm_x3_grid<TL>(M, N)), dim3(TL::THREADS), \
                     0, st, Af, lda, W.x, ldw, W.wps, M, N, K, ep)
#define TVR_X2_LAUNCH(E, TL)                                                                         \
  hipLaunchKernelGGL((gemm_x2f16_nt_kernel<E, TL>), dim3(gemm_x2_grid<TL>(M, N)), dim3(TL::THREADS), 0, \
                     st, Af, lda, W.h, ldw, W.wps, acc_scale, flag, M, N, K, ep)
#define TVR_GEMM_PICK(E)                                                          \
  if (W.h) {                                                                      \
    if (large) TVR_X2_LAUNCH(E, X2Large); else TVR_X2_LAUNCH(E, X2Small);         \
  } else if (W.x) {                                                               \
    if (large) TVR_X3_LAUNCH(E, X3Large); else TVR_X3_LAUNCH(E, X3Small);         \
  } else {                                                                        \
    if (large) TVR_GEMM_LAUNCH(E, TileLarge); else TVR_GEMM_LAUNCH(E, TileSmall); \
  }
    switch (epi) {
      case EPI_BIAS: TVR_GEMM_PICK(EPI_BIAS); break;
      case EPI_SPLIT_GELU: TVR_GEMM_PICK(EPI_SPLIT_GELU); break;
      default: TVR_GEMM_PICK(EPI_RESID); break;
    }
#undef TVR_GEMM_PICK
#undef TVR_X2_LAUNCH
#undef TVR_X3_LAUNCH
#undef TVR_GEMM_LAUNCH
  }
  TVR_HIP(hipGetLastError());
  if (ev0 && ev1) {
    TVR_HIP(hipEventRecord(ev1, st));
    // minimal operand bytes: W read once (fp32 4, 3 bf16 planes 6, 2 fp16 planes 4, bf16 2 B per element),
    // A once in its format (fp32 / x2f16 4, bf16 2), C once as fp32
    // (EPI_STATS: the per-tile statistics records instead of C)
    const double wbytes = W.x ? 6.0 : (a_fmt == ACT_BF16 || a_fmt == ACT_F16 ? 2.0 : 4.0);
    const double abytes = a_fmt == ACT_BF16 || a_fmt == ACT_F16 ? 2.0 : 4.0;
    const double cbytes = epi == EPI_STATS ? 4.0 * M * (double)ep.stats_tiles * (2 + 2 * ep.stats_k)
                                           : 4.0 * M * (double)N;
    const int kind = epi == EPI_SPLIT_GELU_ACT ? (int)EPI_SPLIT_GELU : epi == EPI_STATS ? (int)EPI_BIAS : epi;
    m->prof_recs.push_back({ev0, ev1, kind, 2.0 * M * N * (double)K,
                            abytes * M * (double)K + cbytes + wbytes * N * (double)K});
  }
  return TVR_OK;
}

// W's rows from row r0 on (row stride ld): a launch over a column range of the weights.  The interleaved copy
// pairs rows, so pair r0 / 2 starts at row r0's own offset only for an even r0 (the engine's offsets are
// multiples of d_model, a multiple of 32 on the exact-fp16 path: checked here, not assumed).
int w_from_row(const MatW& W, int r0, int ld, MatW& out) {
  if (W.hil && (r0 & 1))
    return fail(TVR_ERR_INTERNAL, "gemm: odd weight row offset " + std::to_string(r0) + " into a row-pair-interleaved plane");
  out = W.rows((size_t)r0 * ld);
  return TVR_OK;
}

// TVR_GEMM_BF16: the attention-score columns [0, 2d) of the linearised entry
// run on fp16 operands when they are whole 256-column tiles (else 0: bf16)
int lin_qk_cols(const tvr_config& c) { return (2 * c.d_model) % 256 == 0 ? 2 * c.d_model : 0; }

// The linearised entry layer's model constants (lin_entry.hpp) for the
// current planar mode: per layer l = 1 .. L-2, Wsc = W1[l] W_O[l-1] on the
// exact-product fp32 MFMA GEMM, its planes (X2F16: per-layer power-of-two
// scale, as the weights), and c1[l] = row sums of W1[l] in fp64.
int ensure_lin(tvr_model* m, hipStream_t st) {
  const int fmt = act_fmt(m);
  if (fmt == ACT_F32) return fail(TVR_ERR_INVALID, "lin entry: needs a planar GEMM mode");
  if (m->lin_planes && m->lin_mode == m->gemm_mode) return TVR_OK;
  if (m->lin_failed_mode == m->gemm_mode)  // remembered: no sync, no allocation attempt per sweep
    return fail(TVR_ERR_NOMEM, "lin entry: the W1 W_O planes do not fit (earlier attempt)");
  const tvr_config& c = m->cfg;
  const int L = c.n_layers, d = c.d_model, H = c.n_heads, dh = c.d_head, N = m->D1;
  if (L < 3) return fail(TVR_ERR_INVALID, "lin entry: needs >= 3 layers");
  TVR_HIP(hipStreamSynchronize(st));
  if (m->lin_planes) TVR_HIP(hipFree(m->lin_planes));
  if (m->lin_c1) TVR_HIP(hipFree(m->lin_c1));
  m->lin_planes = nullptr;
  m->lin_c1 = nullptr;
  const int KP = (dh + 31) / 32 * 32, npl = fmt == ACT_X2F16 ? 2 : 1;
  const size_t per = (size_t)H * N * KP;
  float *wt = nullptr, *sc = nullptr;
  unsigned* d_max = nullptr;
  auto cleanup = [&]() {
    if (wt) (void)hipFree(wt);
    if (sc) (void)hipFree(sc);
    if (d_max) (void)hipFree(d_max);
  };
  // The split-K partials workspace is released for a second attempt; the
  // planes are kept only if that workspace can be re-reserved at its former
  // size afterwards (the sweep's split-K launches need it back: otherwise they
  // would fail with NOMEM where the full-GEMM entry succeeds).
  const size_t splitk_had = m->splitk_bytes;
  for (int attempt = 0;; ++attempt) {
    bool ok = hipMalloc(&m->lin_planes, (size_t)(L - 2) * npl * per * sizeof(uint16_t)) == hipSuccess &&
              hipMalloc(&m->lin_c1, (size_t)L * N * sizeof(float)) == hipSuccess &&
              hipMalloc(&wt, (size_t)d * d * sizeof(float)) == hipSuccess &&
              hipMalloc(&sc, (size_t)N * d * sizeof(float)) == hipSuccess &&
              hipMalloc(&d_max, sizeof(unsigned)) == hipSuccess;
    if (ok && attempt > 0 && splitk_had > 0) {
      (void)hipGetLastError();
      ok = hipMalloc(&m->splitk_ws, splitk_had) == hipSuccess;
      if (ok) {
        m->splitk_bytes = splitk_had;
      } else {
        m->splitk_ws = nullptr;
      }
    }
    if (ok) break;
    (void)hipGetLastError();
    cleanup();
    wt = sc = nullptr;
    d_max = nullptr;
    if (m->lin_planes) (void)hipFree(m->lin_planes);
    if (m->lin_c1) (void)hipFree(m->lin_c1);
    m->lin_planes = nullptr;
    m->lin_c1 = nullptr;
    if (attempt == 0 && m->splitk_ws) {
      (void)hipFree(m->splitk_ws);
      m->splitk_ws = nullptr;
      m->splitk_bytes = 0;
      continue;
    }
    m->lin_failed_mode = m->gemm_mode;
    return fail(TVR_ERR_NOMEM, "lin entry: the W1 W_O planes do not fit");
  }
  m->lin_scale.assign(L, 1.0f);
  int rc = TVR_OK;
  for (int l = 1; l <= L - 2 && rc == TVR_OK; ++l) {
    hipLaunchKernelGGL(transpose_kernel, dim3((d + 31) / 32, (d + 31) / 32), dim3(32, 8), 0, st,
                       m->layers[l - 1].w2, m->K2, wt, d);
    GemmEpi e{};
    e.out0 = sc;
    e.ld0 = d;
    rc = launch_gemm(EPI_BIAS, m->layers[l].w1, d, ACT_F32, MatW{wt}, d, N, d, d, e, st);
    if (rc != TVR_OK) break;
    float scale = 1.0f;
    {  // X2F16: one power-of-two scale from max |Wsc|; BF16: from max |Wsc| over the Q / K rows (fp16 there)
      unsigned hm = 0;
      hipError_t e2 = hipMemsetAsync(d_max, 0, sizeof(unsigned), st);
      if (e2 == hipSuccess) {
        const size_t n_abs = fmt == ACT_X2F16 ? (size_t)N * d : (size_t)2 * d * d;
        hipLaunchKernelGGL(absmax_kernel, dim3(1024), dim3(256), 0, st, sc, n_abs, d_max);
        e2 = hipGetLastError();
      }
      if (e2 == hipSuccess) e2 = hipMemcpyAsync(&hm, d_max, sizeof(unsigned), hipMemcpyDeviceToHost, st);
      if (e2 == hipSuccess) e2 = hipStreamSynchronize(st);
      if (e2 != hipSuccess) {
        rc = fail(TVR_ERR_HIP, std::string("lin entry: ") + hipGetErrorString(e2));
        break;
      }
      float v;
      std::memcpy(&v, &hm, sizeof(v));
      scale = x2_weight_scale(v);
    }
    if (fmt == ACT_X2F16) {
      hipLaunchKernelGGL(lin_planes_kernel<ACT_X2F16>, dim3(4096), dim3(256), 0, st, sc, N, H, dh, KP, scale,
                         m->lin_planes + (size_t)(l - 1) * npl * per, 0);
    } else {  // fp16 Q / K rows when they fill whole 256-column tiles of lin_entry_kernel (every Pythia but tiny)
      const int n_qk = lin_qk_cols(c);
      if (n_qk == 0) scale = 1.0f;
      hipLaunchKernelGGL(lin_planes_kernel<ACT_BF16>, dim3(4096), dim3(256), 0, st, sc, N, H, dh, KP, scale,
                         m->lin_planes + (size_t)(l - 1) * npl * per, n_qk);
    }
    m->lin_scale[l] = scale;
    hipLaunchKernelGGL(rowsum_kernel, dim3((N + 3) / 4), dim3(256), 0, st, m->layers[l].w1, N, d,
                       m->lin_c1 + (size_t)l * N);
    if (hipGetLastError() != hipSuccess) rc = fail(TVR_ERR_HIP, "lin entry: plane build launch failed");
  }
  if (rc == TVR_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(TVR_ERR_HIP, "lin entry: build failed");
  cleanup();
  if (rc != TVR_OK) {
    (void)hipFree(m->lin_planes);
    (void)hipFree(m->lin_c1);
    m->lin_planes = nullptr;
    m->lin_c1 = nullptr;
    return rc;
  }
  m->lin_kp = KP;
  m->lin_mode = m->gemm_mode;
  return TVR_OK;
}

// dst[r] = src[r] - mean(src[r]) over rows of d floats (src == dst allowed): center_rows_kernel's float4 form
// where both pointers are 16-byte aligned and d % 4 == 0, else the element-wise one (a caller's offset view)
int launch_center_rows(const float* src, float* dst, int rows, int d, hipStream_t st) {
  if (rows <= 0) return TVR_OK;
  const bool v4 = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0 && d % 4 == 0;
  const dim3 grid((rows + 3) / 4), block(256);
  if (v4)
    hipLaunchKernelGGL(center_rows_kernel<true>, grid, block, 0, st, src, dst, rows, d);
  else
    hipLaunchKernelGGL(center_rows_kernel<false>, grid, block, 0, st, src, dst, rows, d);
  TVR_HIP(hipGetLastError());
  return TVR_OK;
}

// y: fp32 [rows][ldy] (ACT_F32) or a planar activation format
// copy: rows < copy_rows of x also go there unchanged (same stride; a fused
// sweep's clean rows into the trace's hook_resid_pre)
// g1 / g2 / y2 (x2f16, exact-fp16 weights): y = LNPre(x) * g1 and y2 = LNPre(x) * g2 (range-checked)
int launch_lnpre(const float* x, int ldx, const int32_t* idx, void* y, int ldy, int rows,
                 int d, float eps, int fmt, hipStream_t st, tvr_model* m = nullptr, float2* stats = nullptr,
                 float* copy = nullptr, int copy_rows = 0, const float* g1 = nullptr, const float* g2 = nullptr,
                 void* y2 = nullptr) {
  if (rows <= 0) return TVR_OK;
  ProfSpan ps(m, st);
  if (d % 4 != 0 || ldx % 4 != 0 || ldy % 4 != 0)
    return fail(TVR_ERR_UNSUPPORTED, "lnpre: d and strides must be multiples of 4");
  // act_col / act_ps address whole 32-column groups: plane 1 of a partial last group would lie past the row
  if (fmt == ACT_X2F16I && (d % 32 != 0 || ldy % 32 != 0))
    return fail(TVR_ERR_UNSUPPORTED, "lnpre: the interleaved layout needs d and ldy to be multiples of 32");
  if (g1 && (!act_is_x2(fmt) || (y2 && !g2) || !m))
    return fail(TVR_ERR_INTERNAL, "lnpre: the gamma-scaled rows are an x2f16 model path");
  const int rows_per_block = 4;
  const dim3 grid((rows + rows_per_block - 1) / rows_per_block), block(64 * rows_per_block);
  // the row in registers: 10 float4 per lane up to d = 2560, 20 up to 5120 (d % 256 == 0), else three passes
  const int nv = d % 256 != 0 ? 0 : d <= 2560 ? 10 : d <= 5120 ? 20 : 0;
#define TVR_LNPRE(F, NV, ...) \
  hipLaunchKernelGGL((lnpre_kernel<F, NV>), grid, block, 0, st, x, ldx, idx, y, ldy, rows, d, eps, stats, copy, copy_rows, __VA_ARGS__)
#define TVR_LNPRE_NV(F, ...)                 \
  if (nv == 10) {                            \
    TVR_LNPRE(F, 10, __VA_ARGS__);           \
  } else if (nv == 20) {                     \
    TVR_LNPRE(F, 20, __VA_ARGS__);           \
  } else {                                   \
    TVR_LNPRE(F, 0, __VA_ARGS__);            \
  }
  if (fmt == ACT_X2F16) {
    TVR_LNPRE_NV(ACT_X2F16, g1, g2, y2, m ? m->range_flag : nullptr);
  } else if (fmt == ACT_X2F16I) {
    TVR_LNPRE_NV(ACT_X2F16I, g1, g2, y2, m ? m->range_flag : nullptr);
  } else if (fmt == ACT_BF16) {
    TVR_LNPRE_NV(ACT_BF16, nullptr, nullptr, nullptr, nullptr);
  } else {
    TVR_LNPRE_NV(ACT_F32, nullptr, nullptr, nullptr, nullptr);
  }
#undef TVR_LNPRE_NV
#undef TVR_LNPRE
  TVR_HIP(hipGetLastError());
  // fp32 rows in, rows out in the activation format (x2f16 / fp32 4 B; bf16 2 + the fp16 plane 2 B per element;
  // the gamma-scaled pair two x2f16 rows)
  ps.done(TVR_HBM_LNPRE, (double)rows * d * (y2 ? 12.0 : 8.0) +
                             (copy ? (double)std::min(rows, copy_rows) * d * 4.0 : 0.0));
  return TVR_OK;
}

// Activation buffers of one launch sequence.  In the planar modes xn and a2
// hold the model's activation format `fmt` (split.hpp) in the same bytes.
struct Acts {
  float* resid;   // [R][d]
  float* xn;      // [R][d]
  float* qkv;     // [R][3d]
  float* a2;      // [R][K2]  (z | gelu(mlp-in))
  int fmt;
  // exact-fp16 weights (use_x16): xn holds LNPre(resid) * gamma1 and xn2 [R][d] LNPre(resid) * gamma2
  float* xn2 = nullptr;
  // a fused clean + patch sweep: rows < mirror_rows (the clean rows) of the
  // layer's resid_pre (LayerNorm's input) and qkv (the QKV epilogue's fp32
  // columns) are also written to the trace by the kernels producing them
  float* resid_mirror = nullptr;
  float* qkv_mirror = nullptr;
  int mirror_rows = 0;
  // head-set sites with patches at the layer being run (tvr_patch_sweep_sets): applied to a2's z columns
  // and resid between the attention and the O + MLP-out GEMM (apply_headset); hs_n == 0: none
  const HeadsetItem* hs_items = nullptr;
  const HeadsetPatch* hs_patches = nullptr;
  const float* hs_vectors = nullptr;
  int hs_n = 0, hs_max_rows = 0;
  double hs_bytes = 0.0;  // algorithmic bytes of the launch (profiling)
  // knockout sites with members at the layer being run (tvr_patch_sweep_knockout): their last rows' z slices
  // are recomputed from qkv / ko_cache between the attention and apply_headset (apply_knockout); ko_n == 0: none
  const KnockoutItem* ko_items = nullptr;
  const uint32_t* ko_masks = nullptr;
  const SeqDesc* ko_seqs = nullptr;  // the launch's sequence descriptors (the items index them)
  const float* ko_cache = nullptr;   // the clean K/V of the prefixes, as the attention launch reads it
  int ko_n = 0, ko_max_keys = 0;
  double ko_bytes = 0.0;
};

// z: the z columns of a2 (fp32 or activation format fmt); zf: optional fp32 copy [rows][d].
// attention_mfma_kernel (one wave per (sequence, head), fp32 MFMA, no LDS) for
// the Pythia head sizes d_head 16 (tiny), 64, 80, 128 with rotary_dim =
// d_head / 4 (every Pythia: rotary_pct 0.25); check_config rejects the rest.
// row_from: sequences [row_from, n_seqs) have exactly one query row (their
// last: q0 = n - 1) and go to attention_row_kernel (HG heads per wave).
bool row_attention_ok(const tvr_config& c) {
  const int hg = c.d_head == 128 ? 2 : 4;
  return c.n_heads % hg == 0 && (c.d_head == 16 || c.d_head == 64 || c.d_head == 80 || c.d_head == 128);
}

int launch_attention(tvr_model* m, const float* qkv, const float* cache_qkv, const SeqDesc* d_seqs,
                     int n_seqs, int maxT, void* z, int fmt, float* zf, hipStream_t st, bool zf_last = false,
                     int zf_rows = INT_MAX, int row_from = INT_MAX, const float* cos_t = nullptr,
                     const float* sin_t = nullptr) {
  if (n_seqs <= 0) return TVR_OK;
  const tvr_config& c = m->cfg;
  // the rotary tables: the model's, or a caller's of the same layout (tvr_attention)
  const float* rot_cos = cos_t ? cos_t : m->rot_cos;
  const float* rot_sin = sin_t ? sin_t : m->rot_sin;
  const int d = c.d_model;
  const float inv_scale = 1.0f / std::sqrt((float)c.d_head);
  const int dh = c.d_head;
  if (row_from < n_seqs && row_attention_ok(c) && env_flag("TVR_ROW_ATTN")) {  // TVR_ROW_ATTN=0: A/B, tests
    const int nr = n_seqs - row_from, hg = dh == 128 ? 2 : 4;
    const dim3 rg((nr * (c.n_heads / hg) + 3) / 4), rb(256);
#define TVR_ATTR(F, DHV)                                                                                         \
  hipLaunchKernelGGL((attention_row_kernel<F, DHV>), rg, rb, 0, st, qkv, 3 * d, cache_qkv, 3 * d, d_seqs, row_from, \
                     nr, c.n_heads, z, m->K2, zf, d, zf_last ? 1 : 0, zf_rows, m->range_flag, rot_cos, rot_sin, \
                     d, inv_scale)
#define TVR_ATTR_DH(F)                                                                         \
  if (dh == 16) { TVR_ATTR(F, 16); } else if (dh == 64) { TVR_ATTR(F, 64); }                   \
  else if (dh == 80) { TVR_ATTR(F, 80); } else { TVR_ATTR(F, 128); }
    if (fmt == ACT_X2F16) {
      TVR_ATTR_DH(ACT_X2F16);
    } else if (fmt == ACT_X2F16I) {
      TVR_ATTR_DH(ACT_X2F16I);
    } else if (fmt == ACT_BF16) {
      TVR_ATTR_DH(ACT_BF16);
    } else {
      TVR_ATTR_DH(ACT_F32);
    }
#undef TVR_ATTR_DH
#undef TVR_ATTR
    TVR_HIP(hipGetLastError());
    n_seqs = row_from;  // the MFMA kernel takes the rest (below)
    if (n_seqs <= 0) return TVR_OK;
  }
  const int pairs = n_seqs * c.n_heads;
  const dim3 grid((pairs + ATTM_WAVES - 1) / ATTM_WAVES), block(64 * ATTM_WAVES);
  // key tiles in registers: 1 / 2 / 4 / 8, or 0 = longer than 128 (chunked online softmax)
  const int kt = (maxT + 15) / 16, nkt = kt <= 1 ? 1 : kt <= 2 ? 2 : kt <= 4 ? 4 : kt <= 8 ? 8 : 0;
  // one key tile: K / V slices staged through LDS by LDS-DMA (default, 2); TVR_ATT_STAGE=1 stages Q as
  // well, 0 loads directly (A/B: profiles/r03/attention_stage_ab.txt)
  const char* se = getenv("TVR_ATT_STAGE");
  const int stage = se && std::string(se) == "0" ? 0 : se && std::string(se) == "1" ? 1 : 2;
  // two key tiles: V staged through LDS (STAGE 3); TVR_ATT_VSTAGE=0 loads it directly (A/B)
  const bool vstage = env_flag("TVR_ATT_VSTAGE");  // read per launch, as TVR_ATT_STAGE (in-process A/B tests)
#define TVR_ATTM(F, DHV, NK, ...)                                                                                   \
  hipLaunchKernelGGL((attention_mfma_kernel<F, DHV, NK __VA_OPT__(,) __VA_ARGS__>), grid, block, 0, st, qkv, 3 * d, cache_qkv, 3 * d, d_seqs, \
                     n_seqs, c.n_heads, z, m->K2, zf, d, zf_last ? 1 : 0, zf_rows, m->range_flag, rot_cos, rot_sin, d, \
                     inv_scale)
#define TVR_ATTM_NK(F, DHV)                                                                     \
  if (nkt == 1 && stage == 1) TVR_ATTM(F, DHV, 1, (DHV <= 80 ? 1 : 0)); /* d_head 128: 98 KB, not staged */ \
  else if (nkt == 1 && stage == 2) TVR_ATTM(F, DHV, 1, (DHV <= 80 ? 2 : 0));                  \
  else if (nkt == 1) TVR_ATTM(F, DHV, 1);                                                       \
  else if (nkt == 2 && vstage) TVR_ATTM(F, DHV, 2, 3);                                          \
  else if (nkt == 2) TVR_ATTM(F, DHV, 2);                                                       \
  else if (nkt == 4) TVR_ATTM(F, DHV, 4);                                                       \
  else if (nkt == 8) TVR_ATTM(F, DHV, 8);                                                       \
  else TVR_ATTM(F, DHV, 0)
#define TVR_ATTM_DH(F)                                                                          \
  if (dh == 16) { TVR_ATTM_NK(F, 16); } else if (dh == 64) { TVR_ATTM_NK(F, 64); }              \
  else if (dh == 80) { TVR_ATTM_NK(F, 80); } else { TVR_ATTM_NK(F, 128); }
  if (fmt == ACT_X2F16) {
    TVR_ATTM_DH(ACT_X2F16);
  } else if (fmt == ACT_X2F16I) {
    TVR_ATTM_DH(ACT_X2F16I);
  } else if (fmt == ACT_BF16) {
    TVR_ATTM_DH(ACT_BF16);
  } else {
    TVR_ATTM_DH(ACT_F32);
  }
#undef TVR_ATTM_DH
#undef TVR_ATTM_NK
#undef TVR_ATTM
  TVR_HIP(hipGetLastError());
  return TVR_OK;
}

// attention_pattern_kernel over n_layers slabs of `qkv` (slab stride layer_stride floats, rows of 3 d floats):
// one wave per (sequence, head), the layer on grid.y.  max_keys: the longest qpos + 1 (sizes the LDS).
// Everything the kernel cannot take is refused here, before the launch.
int launch_pattern(tvr_model* m, const char* fn, const float* qkv, size_t layer_stride, int n_layers,
                   const PatternSeq* d_seqs, int n_seq, int max_keys, const int32_t* d_cls, int n_classes,
                   float* out_pattern, int ld, float* out_mass, const float* cos_t, const float* sin_t,
                   hipStream_t st) {
  const tvr_config& c = m->cfg;
  const int d = c.d_model, dh = c.d_head;
  const size_t lds = pattern_lds_bytes(dh, max_keys);
  if (!(dh == 16 || dh == 64 || dh == 80 || dh == 128) || c.rotary_dim * 4 != dh)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": the pattern kernel covers d_head 16 / 64 / 80 / 128 with "
                                                       "rotary_dim = d_head / 4");
  if (lds > 64 * 1024)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": " + std::to_string(max_keys) + " keys do not fit the "
                                                       "kernel's 64 KiB of LDS scores");
  if ((int64_t)n_seq * c.n_heads > INT_MAX || n_layers > 65535)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": too many (sequence, head) pairs or layers for one launch");
  const float* rot_cos = cos_t ? cos_t : m->rot_cos;
  const float* rot_sin = sin_t ? sin_t : m->rot_sin;
  const float inv_scale = 1.0f / std::sqrt((float)dh);
  const dim3 grid((unsigned)(n_seq * c.n_heads), (unsigned)n_layers), block(64);
#define TVR_PATTERN(DHV)                                                                                          \
  hipLaunchKernelGGL((attention_pattern_kernel<DHV>), grid, block, lds, st, qkv, layer_stride, 3 * d, d_seqs,      \
                     c.n_heads, d_cls, n_classes, out_pattern, ld, out_mass, rot_cos, rot_sin, d, inv_scale)
  if (dh == 16) { TVR_PATTERN(16); } else if (dh == 64) { TVR_PATTERN(64); }
  else if (dh == 80) { TVR_PATTERN(80); } else { TVR_PATTERN(128); }
#undef TVR_PATTERN
  TVR_HIP(hipGetLastError());
  return TVR_OK;
}

// The argument checks tvr_attention_pattern and tvr_trace_capture_pattern share (host only); `fn` prefixes
// the message.  n_cls: entries of cls.
int check_pattern_args(const char* fn, const int32_t* cls, int n_cls, int32_t n_classes, const float* out_pattern,
                       const float* out_mass) {
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!out_pattern && !out_mass) return bad("out_pattern and out_mass are both null");
  if (out_mass && !cls) return bad("out_mass needs cls");
  if (cls) {
    if (n_classes <= 0 || n_classes > PATTERN_MAX_CLASSES)
      return bad("n_classes must be in [1, " + std::to_string(PATTERN_MAX_CLASSES) + "]");
    for (int r = 0; r < n_cls; ++r)
      if (cls[r] < -1 || cls[r] >= n_classes)
        return bad("class of row " + std::to_string(r) + " outside [-1, n_classes)");
  }
  return TVR_OK;
}

// check_pattern_args for tvr_attention_source and tvr_trace_source_attribution: the same rules on out_src / out_cls.
int check_source_args(const char* fn, const int32_t* cls, int n_cls, int32_t n_classes, const float* out_src,
                      const float* out_cls) {
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!out_src && !out_cls) return bad("out_src and out_cls are both null");
  if (out_cls && !cls) return bad("out_cls needs cls");
  if (cls) {
    if (n_classes <= 0 || n_classes > PATTERN_MAX_CLASSES)
      return bad("n_classes must be in [1, " + std::to_string(PATTERN_MAX_CLASSES) + "]");
    for (int r = 0; r < n_cls; ++r)
      if (cls[r] < -1 || cls[r] >= n_classes)
        return bad("class of row " + std::to_string(r) + " outside [-1, n_classes)");
  }
  return TVR_OK;
}

// head_attribution_kernel over n_layers layers from layer0 (logit_attribution.hpp): grid (chunks of 16 rows, H,
// layers).  z rows: slab lz at z + lz * z_lstride, row d_zrows[i] (null: i).  out[(i * n_layers + lz) * H + h].
// Timed under TVR_HBM_CAPTURE: per layer W_O as each chunk of 16 rows reads it, the z and direction rows, out.
int launch_head_attribution(tvr_model* m, const char* fn, const float* dirs, int n, const float* z, size_t z_lstride,
                            const int32_t* d_zrows, int layer0, int n_layers, float* out, hipStream_t st) {
  const tvr_config& c = m->cfg;
  const int d = c.d_model, dh = c.d_head, H = c.n_heads;
  const int chunks = (n + ATTR_CHUNK - 1) / ATTR_CHUNK;
  if (!(dh == 16 || dh == 64 || dh == 80 || dh == 128) || d % 16 != 0)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": the attribution kernel covers d_head 16 / 64 / 80 / 128");
  if (H > 65535 || n_layers > 65535)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": too many heads or layers for one launch");
  ProfSpan ps(m, st);
  const dim3 grid((unsigned)chunks, (unsigned)H, (unsigned)n_layers), block(64 * ATTR_WAVES);
#define TVR_ATTR(NT)                                                                                              \
  hipLaunchKernelGGL((head_attribution_kernel<NT>), grid, block, 0, st, dirs, n, z, z_lstride, d_zrows, m->d_w2s, \
                     layer0, m->K2, out, n_layers, H, d)
  if (dh == 16) { TVR_ATTR(1); } else if (dh == 64) { TVR_ATTR(4); }
  else if (dh == 80) { TVR_ATTR(5); } else { TVR_ATTR(8); }
#undef TVR_ATTR
  TVR_HIP(hipGetLastError());
  ps.done(TVR_HBM_CAPTURE, 4.0 * n_layers * ((double)chunks * d * d + 2.0 * n * d + (double)n * H));
  return TVR_OK;
}

// head_direction_kernel over n_layers layers from layer0 (source_attribution.hpp): out_g[(lz * n + i) * d + col],
// grid (chunks of 16 rows, H, layers).  Timed under TVR_HBM_CAPTURE with the bytes the blocks request: per
// layer W_O once per chunk of 16 rows, the direction rows once per head, G written once.
int launch_head_directions(tvr_model* m, const char* fn, const float* dirs, int n, int layer0, int n_layers,
                           float* out_g, hipStream_t st) {
  const tvr_config& c = m->cfg;
  const int d = c.d_model, dh = c.d_head, H = c.n_heads;
  const int chunks = (n + ATTR_CHUNK - 1) / ATTR_CHUNK;
  if (!(dh == 16 || dh == 64 || dh == 80 || dh == 128) || d % 16 != 0)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": the attribution kernel covers d_head 16 / 64 / 80 / 128");
  if (H > 65535 || n_layers > 65535)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": too many heads or layers for one launch");
  ProfSpan ps(m, st);
  const dim3 grid((unsigned)chunks, (unsigned)H, (unsigned)n_layers), block(64 * ATTR_WAVES);
#define TVR_HDIR(NT)                                                                                              \
  hipLaunchKernelGGL((head_direction_kernel<NT>), grid, block, 0, st, dirs, n, m->d_w2s, layer0, m->K2, out_g, d)
  if (dh == 16) { TVR_HDIR(1); } else if (dh == 64) { TVR_HDIR(4); }
  else if (dh == 80) { TVR_HDIR(5); } else { TVR_HDIR(8); }
#undef TVR_HDIR
  TVR_HIP(hipGetLastError());
  ps.done(TVR_HBM_CAPTURE, 4.0 * n_layers * ((double)chunks * d * d + ((double)H + 1.0) * n * d));
  return TVR_OK;
}

// What launch_source refuses, on the host (tvr_trace_source_attribution checks it before any device call).
int check_source(const tvr_config& c, const char* fn, int n_seq, int n_layers, int max_keys) {
  const int dh = c.d_head;
  if (!(dh == 16 || dh == 64 || dh == 80 || dh == 128) || c.rotary_dim * 4 != dh || c.d_model % 16 != 0)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": the source kernel covers d_head 16 / 64 / 80 / 128 with "
                                                       "rotary_dim = d_head / 4");
  if (source_lds_bytes(dh, max_keys) > 64 * 1024)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": " + std::to_string(max_keys) + " keys do not fit the "
                                                       "kernel's 64 KiB of LDS");
  if ((int64_t)n_seq * c.n_heads > INT_MAX || n_layers > 65535 || c.n_heads > 65535)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": too many (sequence, head) pairs or layers for one launch");
  return TVR_OK;
}

// source_attribution_kernel over n_layers slabs of `qkv` (slab stride layer_stride floats, rows of 3 d floats)
// and of `g` (slab stride g_lstride floats, rows of d floats): one wave per (sequence, head), the layer on
// grid.y; slab l writes layer layer0 + l of outputs that hold out_layers layers.  max_keys: the longest
// qpos + 1 (sizes the LDS).
int launch_source(tvr_model* m, const char* fn, const float* qkv, size_t layer_stride, int n_layers,
                  const PatternSeq* d_seqs, int n_seq, int max_keys, const float* g, size_t g_lstride,
                  const int32_t* d_cls, int n_classes, float* out_src, int ld, float* out_cls, int layer0,
                  int out_layers, const float* cos_t, const float* sin_t, hipStream_t st) {
  const tvr_config& c = m->cfg;
  const int d = c.d_model, dh = c.d_head;
  TVR_TRY(check_source(c, fn, n_seq, n_layers, max_keys));
  const size_t lds = source_lds_bytes(dh, max_keys);
  const float* rot_cos = cos_t ? cos_t : m->rot_cos;
  const float* rot_sin = sin_t ? sin_t : m->rot_sin;
  const float inv_scale = 1.0f / std::sqrt((float)dh);
  const dim3 grid((unsigned)(n_seq * c.n_heads), (unsigned)n_layers), block(64);
#define TVR_SOURCE(DHV)                                                                                           \
  hipLaunchKernelGGL((source_attribution_kernel<DHV>), grid, block, lds, st, qkv, layer_stride, 3 * d, d_seqs,     \
                     c.n_heads, g, g_lstride, d_cls, n_classes, out_src, ld, out_cls, layer0, out_layers, rot_cos, \
                     rot_sin, d, inv_scale)
  if (dh == 16) { TVR_SOURCE(16); } else if (dh == 64) { TVR_SOURCE(64); }
  else if (dh == 80) { TVR_SOURCE(80); } else { TVR_SOURCE(128); }
#undef TVR_SOURCE
  TVR_HIP(hipGetLastError());
  return TVR_OK;
}

// One transformer block over the first R rows (Pythia parallel residual):
//   x = LNPre(resid); [qkv | h] = x @ W1^T + b1; z = attn(qkv); resid += [z|gelu h] @ W2^T + b2
// (run_block computes up to z; run_block_out the second projection.)
// The QKV+MLP-in epilogue: Q|K|V fp32 to qkv (row stride 3d), GELU(h) into
// the a2 columns after z (fp32, or the activation format).
GemmEpi epi_qkv_mlpin(tvr_model* m, const float* b1, float* qkv, const Acts& a) {
  const bool planar = a.fmt != ACT_F32;
  const int d = m->cfg.d_model;
  GemmEpi e{};
  e.bias = b1;
  e.out0 = qkv;
  e.ld0 = 3 * d;
  e.n_split = 3 * d;
  e.out0m = a.qkv_mirror;
  e.mirror_rows = a.mirror_rows;
  if (planar) {
    e.out1h = reinterpret_cast<uint16_t*>(a.a2) + act_col_rt(a.fmt, d);  // (the kernels map the columns after it)
    e.ld1h = 2 * m->K2;
    e.ps1h = m->K2;
    e.range_flag = m->range_flag;
  } else {
    e.out1 = a.a2 + d;
    e.ld1 = m->K2;
  }
  return e;
}

// Algorithmic bytes of one attention launch: Q of the queried rows and K, V of
// every row of the launch (fp32 qkv), z out in the activation format, plus the
// fp32 hook_z copy when one is written (trace / capture).  The shared prefix
// rows read from the trace or a leader are not counted.
double attention_bytes(int d, int q_rows, int kv_rows, int fmt, int zf_rows) {
  return ((double)q_rows * d + 2.0 * kv_rows * d) * 4.0 + (double)q_rows * d * (fmt == ACT_BF16 ? 2.0 : 4.0) +
         (double)zf_rows * d * 4.0;
}

// W1 GEMM over LayerNorm outputs xn (a.fmt), columns [c0, c0 + N) of W1, with
// an epilogue ep already addressed to column c0 (EPI_SPLIT_GELU_ACT planar /
// EPI_SPLIT_GELU fp32).  TVR_GEMM_BF16 runs the attention-score columns
// (Q, K: [0, 2d)) on the fp16 operands instead (W1's fp16 Q / K plane, xn's
// fp16 plane 1: store_ln4) with plain fp32 stores, the rest on bf16.
// xn2 (use_x16): xn / xn2 are LNPre rows scaled by gamma1 / gamma2, and the GEMM runs on the raw W1 rows
// (one exact fp16 plane): the Q | K | V columns [0, 3d) read xn, the MLP-in columns xn2 — per tile in one
// launch when the boundary falls on a 256-column tile edge of the launch, else as two launches.
int launch_w1(tvr_model* m, int l, const void* xn, int M, int c0, int N, const GemmEpi& ep, hipStream_t st,
              const void* xn2 = nullptr) {
  const int d = m->cfg.d_model;
  const int fmt = xn2 ? acts_fmt(m) : act_fmt(m);  // (the gamma-scaled pair: the sweep buffers xn / xn2)
  const int epi = fmt != ACT_F32 ? EPI_SPLIT_GELU_ACT : EPI_SPLIT_GELU;
  if (xn2) {
    if (!use_x16(m) || !act_is_x2(fmt)) return fail(TVR_ERR_INTERNAL, "launch_w1: gamma-scaled rows off the x16 path");
    MatW W;
    TVR_TRY(w_from_row(m->w1x[l], c0, d, W));
    const int qkv_end = 3 * d - c0;  // first column of the launch that reads xn2
    if (qkv_end <= 0)
      return launch_gemm(epi, xn2, d, fmt, W, d, M, N, d, ep, st, m);
    if (qkv_end >= N)
      return launch_gemm(epi, xn, d, fmt, W, d, M, N, d, ep, st, m);
    if (qkv_end % 256 == 0) {
      GemmEpi e = ep;
      e.a2 = static_cast<const uint16_t*>(xn2);
      e.a2_col = qkv_end;
      return launch_gemm(epi, xn, d, fmt, W, d, M, N, d, e, st, m);
    }
    // two launches: columns [c0, 3d) below the GELU split, then the MLP-in columns (their GELU outputs and raw
    // pre-activations are indexed from n_split, which becomes 0)
    GemmEpi e1 = ep;
    e1.n_split = std::min(ep.n_split, qkv_end);
    TVR_TRY(launch_gemm(epi, xn, d, fmt, W, d, M, qkv_end, d, e1, st, m));
    GemmEpi e2 = ep;
    e2.bias = ep.bias ? ep.bias + qkv_end : nullptr;
    e2.out0 = ep.out0 ? ep.out0 + qkv_end : nullptr;
    if (ep.out0m) e2.out0m = ep.out0m + qkv_end;
    e2.n_split = ep.n_split - qkv_end;
    if (e2.n_split < 0) return fail(TVR_ERR_INTERNAL, "launch_w1: MLP-in columns below the GELU split");
    MatW W2;
    TVR_TRY(w_from_row(W, qkv_end, d, W2));
    return launch_gemm(epi, xn2, d, fmt, W2, d, M, N - qkv_end, d, e2, st, m);
  }
  const int nqk = fmt == ACT_BF16 && !m->w1qk.empty() ? std::min(std::max(2 * d - c0, 0), N) : 0;
  if (nqk > 0) {
    GemmEpi e{};
    e.bias = ep.bias;
    e.out0 = ep.out0;
    e.ld0 = ep.ld0;
    e.a_rows = ep.a_rows;
    e.out_rows = ep.out_rows;
    e.out0m = ep.out0m;
    e.mirror_rows = ep.mirror_rows;
    TVR_TRY(launch_gemm(EPI_BIAS, static_cast<const uint16_t*>(xn) + d, d, ACT_F16,
                        m->w1qk[l].rows((size_t)c0 * d), d, M, nqk, d, e, st, m));
    if (nqk == N) return TVR_OK;
  }
  GemmEpi e = ep;
  if (nqk > 0) {
    e.bias = ep.bias ? ep.bias + nqk : nullptr;
    e.out0 = ep.out0 + nqk;
    if (ep.out0m) e.out0m = ep.out0m + nqk;
    e.n_split = ep.n_split - nqk;
  }
  return launch_gemm(epi, xn, d, fmt, m->w1[l].rows((size_t)(c0 + nqk) * d), d, M, N - nqk, d, e, st, m);
}

// The layer's head-set patches (headset_patch.hpp), after the attention has written z and before the
// O + MLP-out GEMM reads it: zero the listed heads' z slices, add their vectors to the residual rows.
int apply_headset(tvr_model* m, const Acts& a, hipStream_t st) {
  if (a.hs_n <= 0) return TVR_OK;
  const tvr_config& c = m->cfg;
  const int d = c.d_model;
  const bool planar = a.fmt != ACT_F32;
  const size_t row_bytes = (size_t)m->K2 * 4;  // fp32 [K2], or halves [2][K2]
  const int slice_bytes = c.d_head * (planar ? 2 : 4);
  const int n_planes = act_is_x2(a.fmt) ? 2 : 1;
  const int il = a.fmt == ACT_X2F16I;
  const size_t plane_bytes = (size_t)m->K2 * 2;
  const dim3 g(a.hs_n, (a.hs_max_rows + HEADSET_ROWS - 1) / HEADSET_ROWS);
  const bool v4 = ((uintptr_t)a.hs_vectors & 15) == 0 && d % 4 == 0;
  ProfSpan ps(m, st);
  if (v4)
    hipLaunchKernelGGL(headset_patch_kernel<true>, g, dim3(HEADSET_THREADS), 0, st, a.hs_items, a.hs_patches,
                       a.hs_vectors, (char*)a.a2, row_bytes, slice_bytes, n_planes, plane_bytes, a.resid, d, il);
  else
    hipLaunchKernelGGL(headset_patch_kernel<false>, g, dim3(HEADSET_THREADS), 0, st, a.hs_items, a.hs_patches,
                       a.hs_vectors, (char*)a.a2, row_bytes, slice_bytes, n_planes, plane_bytes, a.resid, d, il);
  TVR_HIP(hipGetLastError());
  ps.done(TVR_HBM_ENTRY, a.hs_bytes);
  return TVR_OK;
}

// Whether one knockout launch fits the kernel (host only): the head mask and the LDS scores.
int check_knockout(const tvr_config& c, const char* fn, int max_keys) {
  if (c.n_heads > 64)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": the knockout head mask covers 64 heads");
  if (!(c.d_head == 16 || c.d_head == 64 || c.d_head == 80 || c.d_head == 128) || c.rotary_dim * 4 != c.d_head)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": the knockout kernel covers d_head 16 / 64 / 80 / 128 with "
                                                       "rotary_dim = d_head / 4");
  if (knockout_lds_bytes(c.d_head, max_keys) > 64 * 1024)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": " + std::to_string(max_keys) + " keys do not fit the "
                                                       "knockout kernel's 64 KiB of LDS scores");
  return TVR_OK;
}

// The layer's attention knockouts (attention_knockout.hpp), after the attention has written z and before the
// head-set patch and the O + MLP-out GEMM: the listed heads' z slices of the items' last rows are recomputed
// with the blocked keys left out.  One launch, one wave per (item, head); none without items.
int apply_knockout(tvr_model* m, const Acts& a, hipStream_t st, const float* cos_t = nullptr,
                   const float* sin_t = nullptr) {
  if (a.ko_n <= 0) return TVR_OK;
  const tvr_config& c = m->cfg;
  const int d = c.d_model, dh = c.d_head;
  const float* rot_cos = cos_t ? cos_t : m->rot_cos;
  const float* rot_sin = sin_t ? sin_t : m->rot_sin;
  const float inv_scale = 1.0f / std::sqrt((float)dh);
  const size_t lds = knockout_lds_bytes(dh, a.ko_max_keys);
  const dim3 grid((unsigned)a.ko_n * c.n_heads), block(64);
  ProfSpan ps(m, st);
#define TVR_KO(F, DHV)                                                                                              \
  hipLaunchKernelGGL((attention_knockout_kernel<F, DHV>), grid, block, lds, st, a.qkv, 3 * d, a.ko_cache, 3 * d,    \
                     a.ko_seqs, a.ko_items, a.ko_masks, c.n_heads, (void*)a.a2, m->K2, m->range_flag, rot_cos,      \
                     rot_sin, d, inv_scale)
#define TVR_KO_DH(F)                                                                         \
  if (dh == 16) { TVR_KO(F, 16); } else if (dh == 64) { TVR_KO(F, 64); }                     \
  else if (dh == 80) { TVR_KO(F, 80); } else { TVR_KO(F, 128); }
  if (a.fmt == ACT_X2F16) {
    TVR_KO_DH(ACT_X2F16);
  } else if (a.fmt == ACT_X2F16I) {
    TVR_KO_DH(ACT_X2F16I);
  } else if (a.fmt == ACT_BF16) {
    TVR_KO_DH(ACT_BF16);
  } else {
    TVR_KO_DH(ACT_F32);
  }
#undef TVR_KO_DH
#undef TVR_KO
  TVR_HIP(hipGetLastError());
  ps.done(TVR_HBM_ATTENTION, a.ko_bytes);
  return TVR_OK;
}

// zf_last: the fp32 hook_z copy of each sequence's last row only, at row s of zf
int run_block(tvr_model* m, int l, int R, const SeqDesc* d_seqs, int n_seqs, int maxT,
              Acts& a, float* qkv_out, const float* cache_qkv, float* zf, hipStream_t st, bool zf_last = false,
              int zf_rows = INT_MAX, int row_from = INT_MAX) {
  const tvr_config& c = m->cfg;
  const int d = c.d_model;
  const tvr_layer_weights& w = m->layers[l];
  TVR_TRY(launch_lnpre(a.resid, d, nullptr, a.xn, d, R, d, c.ln_eps, a.fmt, st, m, nullptr, a.resid_mirror,
                       a.mirror_rows, a.xn2 ? m->g1[l] : nullptr, a.xn2 ? m->g2[l] : nullptr, a.xn2));
  const GemmEpi e1 = epi_qkv_mlpin(m, w.b1, qkv_out, a);
  TVR_TRY(launch_w1(m, l, a.xn, R, 0, m->D1, e1, st, a.xn2));
  ProfSpan ps(m, st);
  TVR_TRY(launch_attention(m, qkv_out, cache_qkv, d_seqs, n_seqs, maxT, a.a2, a.fmt, zf, st, zf_last, zf_rows,
                           row_from));
  ps.done(TVR_HBM_ATTENTION, attention_bytes(d, R, R, a.fmt, zf ? (zf_last ? n_seqs : std::min(R, zf_rows)) : 0));
  return TVR_OK;
}

// The last layer when only each sequence's LAST row is read afterwards (patch
// sweeps, extraction): every row still needs K and V (they are attended to),
// but Q, the MLP, attention output and the second projection are computed for
// the n_last rows listed in d_last only (~5% of a CIE sweep's FLOPs saved).
// d_seqs must carry q0 = n - 1.  write_out = false skips the second projection
// (nothing downstream reads the final residual).
// row_from: the sequences [row_from, n_seqs) query their last row only (the
// single-query kernel); the ones before it (a fused sweep's clean sequences,
// whose every row the trace keeps: q0 = 0) go to the MFMA kernel.
int run_block_last_rows(tvr_model* m, int l, int R, const SeqDesc* d_seqs, int n_seqs, int maxT, Acts& a,
                        const float* cache_qkv, const int32_t* d_last, int n_last, bool write_out,
                        float* zf, hipStream_t st, bool zf_last = false, int zf_rows = INT_MAX, int row_from = 0) {
  const tvr_config& c = m->cfg;
  const int d = c.d_model;
  const tvr_layer_weights& w = m->layers[l];
  TVR_TRY(launch_lnpre(a.resid, d, nullptr, a.xn, d, R, d, c.ln_eps, a.fmt, st, m, nullptr, a.resid_mirror,
                       a.mirror_rows, a.xn2 ? m->g1[l] : nullptr, a.xn2 ? m->g2[l] : nullptr, a.xn2));
  GemmEpi kv{};  // K | V columns (w1 rows [d, 3d)) for every row (all below n_split: no GELU)
  kv.bias = w.b1 + d;
  kv.out0 = a.qkv + d;
  kv.ld0 = 3 * d;
  kv.n_split = 2 * d;
  TVR_TRY(launch_w1(m, l, a.xn, R, d, 2 * d, kv, st, a.xn2));
  GemmEpi e1 = epi_qkv_mlpin(m, w.b1, a.qkv, a);  // all columns for the last rows, gathered and scattered in place
  e1.a_rows = d_last;
  e1.out_rows = d_last;
  TVR_TRY(launch_w1(m, l, a.xn, n_last, 0, m->D1, e1, st, a.xn2));
  ProfSpan ps(m, st);
  TVR_TRY(launch_attention(m, a.qkv, cache_qkv, d_seqs, n_seqs, maxT, a.a2, a.fmt, zf, st, zf_last, zf_rows,
                           row_from));
  ps.done(TVR_HBM_ATTENTION, attention_bytes(d, n_last, R, a.fmt, zf ? std::min(n_last, zf_rows) : 0));
  if (!write_out) return TVR_OK;
  TVR_TRY(apply_knockout(m, a, st));
  TVR_TRY(apply_headset(m, a, st));  // global row indices, as d_last's (rows the GEMM does not gather are unread)
  GemmEpi e2{};
  e2.bias = w.b2;
  e2.out0 = a.resid;
  e2.ld0 = d;
  e2.resid = a.resid;
  e2.ldr = d;
  e2.a_rows = d_last;
  e2.out_rows = d_last;
  return launch_gemm(EPI_RESID, a.a2, m->K2, a.fmt, use_x16(m) ? m->w2x[l] : m->w2[l], m->K2, n_last, d, m->K2, e2,
                     st, m);
}

int run_block_out(tvr_model* m, int l, int R, Acts& a, hipStream_t st) {
  const int d = m->cfg.d_model;
  const tvr_layer_weights& w = m->layers[l];
  TVR_TRY(apply_knockout(m, a, st));
  TVR_TRY(apply_headset(m, a, st));
  GemmEpi e2{};
  e2.bias = w.b2;
  e2.out0 = a.resid;
  e2.ld0 = d;
  e2.resid = a.resid;
  e2.ldr = d;
  return launch_gemm(EPI_RESID, a.a2, m->K2, a.fmt, use_x16(m) ? m->w2x[l] : m->w2[l], m->K2, R, d, m->K2, e2, st, m);
}

// Final LN + unembed of selected rows + softmax target prob + top-k, chunked.
// Planar modes without requested logits: the unembed GEMM's fused statistics
// epilogue (EPI_STATS: per-tile max / sum exp / top-k candidates / target
// logit, no [rows][V] logits in HBM) + stats_merge_kernel.  Otherwise the
// logits are written (to out_logits, or the scratch) and row_stats_kernel
// reads them back.
bool final_fused(const tvr_model* m, int fmt, const float* out_logits) {
  return fmt != ACT_F32 && !out_logits && m->cfg.d_vocab % 4 == 0;
}
// rows per unembed launch: the fused statistics keep ~200 records per row (no
// [rows][V] logits), so a whole sweep's sites go in one launch (one partly
// empty last round instead of one per 1,024 rows: 37 rounds instead of 52 at
// C3); the logits paths keep 1,024-row chunks of [rows][V] scratch.
int final_chunk(const tvr_model* m, int fmt, const float* out_logits) {
  return final_fused(m, fmt, out_logits) ? 16384 : kFinalChunk;
}
// floats of run_final's scratch for chunks of fc rows
size_t final_scratch_floats(const tvr_model* m, int fmt, int fc, int topk, const float* out_logits) {
  const int V = m->cfg.d_vocab;
  if (final_fused(m, fmt, out_logits)) return (size_t)fc * ((V + 255) / 256) * (2 + 2 * topk) + fc;
  return out_logits ? 0 : (size_t)fc * V;
}

int run_final(tvr_model* m, const float* resid, const int32_t* d_rows, const int32_t* d_targets,
              int n, float* xf, float* scratch, float* out_prob, int32_t* out_topk, int topk,
              float* out_logits, int fmt, hipStream_t st) {
  const tvr_config& c = m->cfg;
  const int d = c.d_model, V = c.d_vocab;
  const bool fused = final_fused(m, fmt, out_logits);
  const int tiles = (V + 255) / 256, chunk = final_chunk(m, fmt, out_logits);
  for (int s = 0; s < n; s += chunk) {
    const int cn = std::min(chunk, n - s);
    // the exact-fp16 unembed: LNPre(x) o gamma_f against the raw W_U (the statistics are invariant to the
    // per-row constant this leaves in the logits; the logits path removes it below)
    const bool xu = use_x16(m) && m->wux.h;
    if (xu) fmt = acts_fmt(m);  // xf: read by the one-plane unembed
    TVR_TRY(launch_lnpre(resid, d, d_rows + s, xf, d, cn, d, c.ln_eps, fmt, st, m, nullptr, nullptr, 0,
                         xu ? m->gf : nullptr));
    if (fused) {
      float* part = scratch;
      float* tlogit = scratch + (size_t)cn * tiles * (2 + 2 * topk);
      GemmEpi e{};
      e.bias = m->b_unembed;
      e.stats = part;
      e.stats_k = topk;
      e.stats_tiles = tiles;
      e.targets = d_targets ? d_targets + s : nullptr;
      e.tlogit = tlogit;
      TVR_TRY(launch_gemm(EPI_STATS, xf, d, fmt, xu ? m->wux : m->wu, d, cn, V, d, e, st, m));
      ProfSpan ps(m, st);
      hipLaunchKernelGGL(stats_merge_kernel, dim3((cn + MERGE_WAVES - 1) / MERGE_WAVES), dim3(64 * MERGE_WAVES), 0,
                         st, part, tiles, topk, tlogit, d_targets ? d_targets + s : nullptr, cn, V,
                         out_prob ? out_prob + s : nullptr, out_topk ? out_topk + (size_t)s * topk : nullptr, topk);
      TVR_HIP(hipGetLastError());
      ps.done(TVR_HBM_ROW_STATS, (double)cn * (tiles * (2.0 + 2.0 * topk) + 1.0) * 4.0);  // the records + target logit
      continue;
    }
    float* lg = out_logits ? out_logits + (size_t)s * V : scratch;
    GemmEpi e{};
    e.bias = m->b_unembed;
    e.out0 = lg;
    e.ld0 = V;
    TVR_TRY(launch_gemm(EPI_BIAS, xf, d, fmt, xu ? m->wux : m->wu, d, cn, V, d, e, st, m));
    if (xu) {
      // TL's W_U' = center_unembed(fold_ln(W_U)): (LNPre(x) o gamma_f) W_U^T + b_U' differs from TL's logits by
      // -LNPre(x) . (the vocab mean of the d-centred rows), one constant per row, and TL's logits have mean 0 over
      // the vocabulary (W_U' and b_U' are centred over it): subtract each row's mean
      TVR_TRY(launch_center_rows(lg, lg, cn, V, st));
    }
    ProfSpan ps(m, st);
    hipLaunchKernelGGL(row_stats_kernel, dim3(cn), dim3(STATS_THREADS), 0, st, lg, V, V,
                       d_targets ? d_targets + s : nullptr, out_prob ? out_prob + s : nullptr,
                       out_topk ? out_topk + (size_t)s * topk : nullptr, topk);
    TVR_HIP(hipGetLastError());
    ps.done(TVR_HBM_ROW_STATS, (double)cn * V * 4.0);  // one fp32 logit row per site
  }
  return TVR_OK;
}

int check_config(const tvr_config& c) {
  if (c.n_layers <= 0 || c.d_model <= 0 || c.n_heads <= 0 || c.d_head <= 0 || c.d_mlp <= 0 ||
      c.d_vocab <= 0 || c.n_ctx <= 0)
    return fail(TVR_ERR_INVALID, "config: all sizes must be positive");
  if (c.n_heads * c.d_head != c.d_model)
    return fail(TVR_ERR_INVALID, "config: n_heads * d_head must equal d_model");
  if (c.rotary_dim < 0 || c.rotary_dim > c.d_head || (c.rotary_dim & 1))
    return fail(TVR_ERR_INVALID, "config: rotary_dim must be even and <= d_head");
  if (c.d_model % GEMM_BK != 0 || (c.d_model + c.d_mlp) % GEMM_BK != 0)
    return fail(TVR_ERR_UNSUPPORTED, "config: d_model and d_model + d_mlp must be multiples of 32");
  if (!(c.d_head == 16 || c.d_head == 64 || c.d_head == 80 || c.d_head == 128) || c.rotary_dim * 4 != c.d_head)
    return fail(TVR_ERR_UNSUPPORTED, "config: the attention kernel covers the Pythia heads: d_head 16 / 64 / 80 / "
                                     "128 with rotary_dim = d_head / 4");
  return TVR_OK;
}

}  // namespace

// ===========================================================================
namespace {
int flush_pending(tvr_trace* t, void* stream);
}  // namespace

extern "C" {

const char* tvr_version(void) {
  return "tvr-mi355x 0.5.0 (gfx950, fp32 MFMA | fp32-accurate 3-plane bf16 / 2-plane fp16 split MFMA | bf16 MFMA)";
}
int32_t tvr_abi_version(void) { return TVR_ABI_VERSION; }
const char* tvr_last_error(void) { return g_last_error.c_str(); }

int tvr_model_create(const tvr_config* cfg, const float* w_embed, const tvr_layer_weights* layers,
                     const float* w_unembed_t, const float* b_unembed, tvr_model** out) {
  if (!cfg || !w_embed || !layers || !w_unembed_t || !out)
    return fail(TVR_ERR_INVALID, "tvr_model_create: null argument");
  TVR_TRY(check_config(*cfg));
  for (int l = 0; l < cfg->n_layers; ++l)
    if (!layers[l].w1 || !layers[l].b1 || !layers[l].w2 || !layers[l].b2)
      return fail(TVR_ERR_INVALID, "tvr_model_create: null weight in layer " + std::to_string(l));
  auto* m = new tvr_model();
  m->cfg = *cfg;
  m->D1 = 3 * cfg->d_model + cfg->d_mlp;
  m->K2 = cfg->d_model + cfg->d_mlp;
  m->w_embed = w_embed;
  m->layers.assign(layers, layers + cfg->n_layers);
  m->w_unembed_t = w_unembed_t;
  m->b_unembed = b_unembed;
  for (int l = 0; l < cfg->n_layers; ++l) {
    m->w1.push_back(MatW{layers[l].w1});
    m->w2.push_back(MatW{layers[l].w2});
  }
  m->wu = MatW{w_unembed_t};
  // TL calculate_sin_cos_rotary: freq = base^(i / (rd/2)), repeated "(2 d)",
  // angle = pos / freq, all in fp32.
  const int rd = std::max(cfg->rotary_dim, 2), n_ctx = cfg->n_ctx;
  std::vector<float> hc((size_t)n_ctx * rd), hs((size_t)n_ctx * rd);
  const int half = rd / 2;
  for (int p = 0; p < n_ctx; ++p)
    for (int i = 0; i < rd; ++i) {
      const float dim = (float)(i % half);
      const float freq = std::pow(cfg->rotary_base, dim / (float)half);
      const float ang = (float)p / freq;
      hc[(size_t)p * rd + i] = std::cos(ang);
      hs[(size_t)p * rd + i] = std::sin(ang);
    }
  std::vector<const float*> w2s(cfg->n_layers);
  for (int l = 0; l < cfg->n_layers; ++l) w2s[l] = layers[l].w2;
  hipError_t e = hipMalloc(&m->rot_cos, hc.size() * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&m->rot_sin, hs.size() * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&m->d_w2s, w2s.size() * sizeof(float*));
  if (e == hipSuccess) e = hipMalloc(&m->range_flag, sizeof(unsigned));
  if (e == hipSuccess) e = hipMemset(m->range_flag, 0, sizeof(unsigned));
  if (e == hipSuccess) e = hipMemcpy(m->rot_cos, hc.data(), hc.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->rot_sin, hs.data(), hs.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->d_w2s, w2s.data(), w2s.size() * sizeof(float*), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    tvr_model_destroy(m);
    return fail(TVR_ERR_HIP, std::string("tvr_model_create: ") + hipGetErrorString(e));
  }
  *out = m;
  return TVR_OK;
}

// Drop the interleaved weight copies (layers: W1 / W2 of every layer; unembed: W_U).  The caller has made sure
// that no launch still reads them.
static void free_w_il(tvr_model* m, bool layers, bool unembed) {
  if (layers) {
    if (m->w_il) (void)hipFree(m->w_il);
    m->w_il = nullptr;
    for (auto& w : m->w1x) w.hil = nullptr;
    for (auto& w : m->w2x) w.hil = nullptr;
  }
  if (unembed) {
    if (m->wu_il) (void)hipFree(m->wu_il);
    m->wu_il = nullptr;
    m->wux.hil = nullptr;
  }
  if (!m->w_il && !m->wu_il) m->w_il_nomem = false;
}

// Bring the interleaved copies in line with the model's state: present exactly while the exact-fp16 path runs
// in the interleaved activation layout (the only reader: launch_gemm's wil form) and TVR_W_LAYOUT allowed them
// at the binding; the unembed's only with its plane bound.  A copy that does not fit is not an error: the
// GEMMs then read the plain planes (w_il_nomem).  On the null stream, synchronised.
static int sync_w_il(tvr_model* m) {
  const bool want = use_x16(m) && m->act_il && m->w_il_wanted && pp_wil_available();
  if (!want) {
    if (m->w_il || m->wu_il) TVR_HIP(hipDeviceSynchronize());
    free_w_il(m, true, true);
    return TVR_OK;
  }
  const tvr_config& c = m->cfg;
  const int L = c.n_layers, d = c.d_model;
  const dim3 grid(4096), block(256);
  bool launched = false;
  if (!m->w_il) {
    const size_t n1 = w_il_halves(m->D1, d), n2 = w_il_halves(d, m->K2);
    if (hipMalloc(&m->w_il, (size_t)L * (n1 + n2) * sizeof(uint16_t)) != hipSuccess) {
      m->w_il = nullptr;
      (void)hipGetLastError();
      m->w_il_nomem = true;
    } else {
      uint16_t* p = m->w_il;
      for (int l = 0; l < L; ++l) {
        hipLaunchKernelGGL(weight_plane_il_kernel, grid, block, 0, 0, m->w1x[l].h, p, (size_t)m->D1, d);
        m->w1x[l].hil = p;
        p += n1;
        hipLaunchKernelGGL(weight_plane_il_kernel, grid, block, 0, 0, m->w2x[l].h, p, (size_t)d, m->K2);
        m->w2x[l].hil = p;
        p += n2;
      }
      launched = true;
    }
  }
  if (m->wux.h && !m->wu_il) {
    if (hipMalloc(&m->wu_il, w_il_halves(c.d_vocab, d) * sizeof(uint16_t)) != hipSuccess) {
      m->wu_il = nullptr;
      (void)hipGetLastError();
      m->w_il_nomem = true;
    } else {
      hipLaunchKernelGGL(weight_plane_il_kernel, grid, block, 0, 0, m->wux.h, m->wu_il, (size_t)c.d_vocab, d);
      m->wux.hil = m->wu_il;
      launched = true;
    }
  }
  if (launched) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      free_w_il(m, true, true);
      return fail(TVR_ERR_HIP, std::string("interleaved weight copies: ") + hipGetErrorString(e));
    }
  }
  return TVR_OK;
}

int32_t tvr_model_weight_layout(const tvr_model* m) {
  if (!m) return -1;
  return (m->w_il ? TVR_W_IL_LAYERS : 0) | (m->wu_il ? TVR_W_IL_UNEMBED : 0) | (m->w_il_nomem ? TVR_W_IL_NOMEM : 0);
}

int tvr_weight_rows_il(const uint16_t* w, uint16_t* out, int32_t N, int32_t K, void* stream) {
  if (!w || !out || N <= 0 || K <= 0 || K % 32 != 0) return fail(TVR_ERR_INVALID, "tvr_weight_rows_il: bad argument");
  const size_t n = w_il_halves(N, K);
  hipLaunchKernelGGL(weight_plane_il_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0,
                     (hipStream_t)stream, w, out, (size_t)N, K);
  TVR_HIP(hipGetLastError());
  return TVR_OK;
}

int tvr_model_destroy(tvr_model* m) {
  if (!m) return TVR_OK;
  (void)hipDeviceSynchronize();
  free_w_il(m, true, true);
  if (m->rot_cos) (void)hipFree(m->rot_cos);
  if (m->rot_sin) (void)hipFree(m->rot_sin);
  if (m->d_w2s) (void)hipFree(m->d_w2s);
  if (m->planes) (void)hipFree(m->planes);
  if (m->lin_planes) (void)hipFree(m->lin_planes);
  if (m->lin_c1) (void)hipFree(m->lin_c1);
  if (m->range_flag) (void)hipFree(m->range_flag);
  if (m->ws) (void)hipFree(m->ws);
  if (m->splitk_ws) (void)hipFree(m->splitk_ws);
  for (auto& r : m->prof_recs) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  for (auto e : m->prof_pool) (void)hipEventDestroy(e);
  for (int i = 0; i < 2; ++i) {
    if (m->staging.buf[i]) (void)hipHostFree(m->staging.buf[i]);
    if (m->staging.done[i]) (void)hipEventDestroy(m->staging.done[i]);
  }
  delete m;
  return TVR_OK;
}

size_t tvr_workspace_bytes(const tvr_model* m) { return m ? m->ws_bytes : 0; }

int32_t tvr_model_get_gemm(const tvr_model* m) { return m ? m->gemm_mode : -1; }

// X2F16 mode: the weight planes again for the current exact-fp16 binding (with / without the w2 planes),
// on the null stream
static int replan_x2f16(tvr_model* m) {
  if (m->gemm_mode != TVR_GEMM_X2F16) return TVR_OK;
  TVR_HIP(hipDeviceSynchronize());  // no launch on any stream may still read the planes about to be freed
  TVR_TRY(tvr_model_set_gemm(m, TVR_GEMM_F32, nullptr));
  return tvr_model_set_gemm(m, TVR_GEMM_X2F16, nullptr);
}

int tvr_model_set_exact16_unembed(tvr_model* m, const uint16_t* wu, const float* gf) {
  if (!m) return fail(TVR_ERR_INVALID, "tvr_model_set_exact16_unembed: null model");
  if (!wu != !gf) return fail(TVR_ERR_INVALID, "tvr_model_set_exact16_unembed: give both arrays or neither");
  if (m->wu_il) TVR_HIP(hipDeviceSynchronize());  // a rebind: no launch may still read the copy about to go
  free_w_il(m, false, true);
  m->wux = wu ? MatW{nullptr, nullptr, wu, 0, 1.0f, true} : MatW{};
  m->gf = gf;
  return sync_w_il(m);
}

int tvr_model_set_exact16(tvr_model* m, const tvr_exact16_layer* layers) {
  if (!m) return fail(TVR_ERR_INVALID, "tvr_model_set_exact16: null model");
  const tvr_config& c = m->cfg;
  // the interleaved copies belong to the planes bound so far: dropped on a rebind and a detach alike (the
  // re-plan below builds the new binding's)
  if (m->w_il || m->wu_il) TVR_HIP(hipDeviceSynchronize());
  free_w_il(m, true, true);
  if (!layers) {
    const bool was = m->x16;
    m->x16 = false;
    m->w1x.clear();
    m->w2x.clear();
    m->g1.clear();
    m->g2.clear();
    return was ? replan_x2f16(m) : TVR_OK;
  }
  for (int l = 0; l < c.n_layers; ++l)
    if (!layers[l].w1 || !layers[l].w2 || !layers[l].g1 || !layers[l].g2)
      return fail(TVR_ERR_INVALID, "tvr_model_set_exact16: null array in layer " + std::to_string(l));
  // the one-plane kernel's staging reads rows of 8-halve chunks and d of 4-float groups (launch_gemm's K / ld
  // checks cover the rest)
  if (c.d_model % 32 != 0 || m->K2 % 32 != 0)
    return fail(TVR_ERR_UNSUPPORTED, "tvr_model_set_exact16: d_model and d_model + d_mlp must be multiples of 32");
  m->w1x.clear();
  m->w2x.clear();
  m->g1.clear();
  m->g2.clear();
  for (int l = 0; l < c.n_layers; ++l) {
    // one plane of the raw values themselves: weight scale 1 (fp16 subnormals reach the matrix cores as
    // they are: tools/denorm_probe.py), no second plane (wps 0 is never read: WX kernels only)
    m->w1x.push_back(MatW{nullptr, nullptr, layers[l].w1, 0, 1.0f, true});
    m->w2x.push_back(MatW{nullptr, nullptr, layers[l].w2, 0, 1.0f, true});
    m->g1.push_back(layers[l].g1);
    m->g2.push_back(layers[l].g2);
  }
  m->x16 = true;
  m->w_il_wanted = w_layout_interleaved();
  return replan_x2f16(m);
}

int tvr_model_set_gemm(tvr_model* m, int32_t mode, void* stream) {
  if (!m) return fail(TVR_ERR_INVALID, "tvr_model_set_gemm: null model");
  if (mode != TVR_GEMM_F32 && mode != TVR_GEMM_X3BF16 && mode != TVR_GEMM_X2F16 && mode != TVR_GEMM_BF16)
    return fail(TVR_ERR_INVALID, "tvr_model_set_gemm: unknown mode " + std::to_string(mode));
  if (mode == m->gemm_mode) return TVR_OK;
  if (mode == TVR_GEMM_BF16 && (m->cfg.d_model % 64 != 0 || m->K2 % 64 != 0))
    return fail(TVR_ERR_UNSUPPORTED, "tvr_model_set_gemm: bf16 needs d_model and d_model + d_mlp multiples of 64");
  const hipStream_t st = (hipStream_t)stream;
  TVR_HIP(hipStreamSynchronize(st));
  // back to plain fp32 operands first (frees the previous mode's planes)
  for (auto& w : m->w1) w = MatW{w.f};
  for (auto& w : m->w2) w = MatW{w.f};
  m->w1qk.clear();
  m->wu = MatW{m->wu.f};
  if (m->planes) TVR_HIP(hipFree(m->planes));
  m->planes = nullptr;
  if (m->lin_planes) TVR_HIP(hipFree(m->lin_planes));
  if (m->lin_c1) TVR_HIP(hipFree(m->lin_c1));
  m->lin_planes = nullptr;
  m->lin_c1 = nullptr;
  m->lin_mode = -1;
  m->lin_failed_mode = -1;
  m->gemm_mode = TVR_GEMM_F32;
  TVR_TRY(sync_w_il(m));  // off the exact-fp16 path: the interleaved weight copies go
  if (mode == TVR_GEMM_F32) return TVR_OK;

  const tvr_config& c = m->cfg;
  const int L = c.n_layers;
  const size_t n1 = (size_t)m->D1 * c.d_model, n2 = (size_t)c.d_model * m->K2;
  const size_t nu = (size_t)c.d_vocab * c.d_model;
  const int np = mode == TVR_GEMM_X3BF16 ? 3 : mode == TVR_GEMM_X2F16 ? 2 : 1;
  const size_t nqk = (size_t)2 * c.d_model * c.d_model;  // BF16: W1's Q / K rows as an fp16 plane
  // diagnostic knobs, read per call, for the bf16 bars' negative controls (tests/test_gpu_full_depth.py
  // test_bf16_bars_reject_a_wrong_bf16_path) — never set in production: TVR_DEBUG_BF16_QK=0 drops the fp16
  // Q / K operands (the Q / K columns run on bf16 like the rest), TVR_DEBUG_BF16_TRUNC=1 builds the bf16
  // weight planes by truncation instead of round-to-nearest-even
  const bool bf16_qk16 = env_int("TVR_DEBUG_BF16_QK", 1) != 0;
  const bool bf16_trunc = env_int("TVR_DEBUG_BF16_TRUNC", 0) != 0;
  const size_t total = np * ((mode == TVR_GEMM_X2F16 && m->x16 ? 0 : n1 + n2) * L + nu) +
                       (mode == TVR_GEMM_BF16 && bf16_qk16 ? nqk * L : 0);
  if (hipMalloc(&m->planes, total * sizeof(uint16_t)) != hipSuccess) {
    m->planes = nullptr;
    (void)hipGetLastError();
    return fail(TVR_ERR_NOMEM, "tvr_model_set_gemm: weight planes (" + std::to_string(total * 2) +
                                   " bytes) do not fit");
  }
  // every GEMM weight matrix in order: w1[0], w2[0], ..., w1[L-1], w2[L-1], wu — in X2F16 with exact-fp16
  // weights bound (tvr_model_set_exact16) without the w1 / w2 planes: every QKV + MLP-in, O + MLP-out and
  // linearised-entry G GEMM reads the raw fp16 rows (2.8B: 5.9 + 4.2 GB, 12B: 26 + 19 GB not allocated)
  const bool skip_x16 = mode == TVR_GEMM_X2F16 && m->x16;
  std::vector<MatW*> mats;
  std::vector<size_t> sizes;
  for (int l = 0; l < L && !skip_x16; ++l) {
    mats.push_back(&m->w1[l]);
    sizes.push_back(n1);
    mats.push_back(&m->w2[l]);
    sizes.push_back(n2);
  }
  mats.push_back(&m->wu); sizes.push_back(nu);
  if (mode == TVR_GEMM_BF16 && bf16_qk16) {  // the fp16 Q / K planes: one scale per layer from max |W_QK|
    for (int l = 0; l < L; ++l) {
      mats.push_back(nullptr);
      sizes.push_back(nqk);
    }
  }
  std::vector<float> scale(mats.size(), 1.0f);  // sized after the Q / K entries: one per matrix
  // the planes of every matrix exactly fill the allocation: checked BEFORE any conversion kernel writes
  // (a fp16 Q / K entry is one plane, every other matrix np planes)
  size_t planned = 0;
  for (size_t i = 0; i < mats.size(); ++i) planned += (mats[i] ? (size_t)np : 1) * sizes[i];
  auto drop_planes = [&]() {
    (void)hipFree(m->planes);
    m->planes = nullptr;
    for (auto& w : m->w1) w = MatW{w.f};
    for (auto& w : m->w2) w = MatW{w.f};
    m->w1qk.clear();
    m->wu = MatW{m->wu.f};
  };
  if (planned != total) {
    drop_planes();
    return fail(TVR_ERR_INTERNAL, "tvr_model_set_gemm: planes planned " + std::to_string(planned) +
                                      " != allocated " + std::to_string(total));
  }
  if (mode == TVR_GEMM_X2F16 || mode == TVR_GEMM_BF16) {
    // one power-of-two scale per matrix from its largest magnitude
    unsigned* d_max = nullptr;
    TVR_HIP(hipMalloc(&d_max, mats.size() * sizeof(unsigned)));
    std::vector<unsigned> h_max(mats.size(), 0);
    hipError_t e = hipMemsetAsync(d_max, 0, mats.size() * sizeof(unsigned), st);
    for (size_t i = 0; i < mats.size() && e == hipSuccess; ++i) {
      const float* src = mats[i] ? mats[i]->f : m->w1[i - (mats.size() - L)].f;  // null: layer's Q / K rows
      if (mode == TVR_GEMM_BF16 && mats[i]) continue;
      hipLaunchKernelGGL(absmax_kernel, dim3(1024), dim3(256), 0, st, src, sizes[i], d_max + i);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_max.data(), d_max, mats.size() * sizeof(unsigned),
                                            hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_max);
    if (e != hipSuccess) return fail(TVR_ERR_HIP, std::string("tvr_model_set_gemm: ") + hipGetErrorString(e));
    for (size_t i = 0; i < mats.size(); ++i) {
      float v;
      std::memcpy(&v, &h_max[i], sizeof(v));
      scale[i] = x2_weight_scale(v);
    }
  }
  uint16_t* p = m->planes;
  for (size_t i = 0; i < mats.size(); ++i) {
    const size_t n = sizes[i];
    if (!mats[i]) {  // BF16: layer l's fp16 Q / K plane (the first 2d rows of W1, row stride d)
      const int l = (int)(i - (mats.size() - L));
      const float* f = m->w1[l].f;
      hipLaunchKernelGGL(f16_plane_kernel, dim3(2048), dim3(256), 0, st, f, scale[i], p, n);
      TVR_HIP(hipGetLastError());
      m->w1qk.push_back(MatW{f, nullptr, p, n, scale[i]});
      p += n;
      continue;
    }
    MatW& w = *mats[i];
    if (mode == TVR_GEMM_X3BF16) {
      hipLaunchKernelGGL(split_planes_kernel, dim3(2048), dim3(256), 0, st, w.f, p, n);
      w = MatW{w.f, p, nullptr, n, 1.0f};
    } else if (mode == TVR_GEMM_BF16) {
      hipLaunchKernelGGL(bf16_plane_kernel, dim3(2048), dim3(256), 0, st, w.f, p, n, (int)bf16_trunc);
      w = MatW{w.f, nullptr, p, n, 1.0f};
    } else {
      hipLaunchKernelGGL(split_planes_f16_kernel, dim3(2048), dim3(256), 0, st, w.f, scale[i], p, n);
      w = MatW{w.f, nullptr, p, n, scale[i]};
    }
    TVR_HIP(hipGetLastError());
    p += np * n;
  }
  if ((size_t)(p - m->planes) != total) {
    (void)hipStreamSynchronize(st);
    const size_t written = (size_t)(p - m->planes);
    drop_planes();
    return fail(TVR_ERR_INTERNAL, "tvr_model_set_gemm: planes written " + std::to_string(written) +
                                      " != allocated " + std::to_string(total));
  }
  TVR_HIP(hipMemsetAsync(m->range_flag, 0, sizeof(unsigned), st));
  TVR_HIP(hipStreamSynchronize(st));
  m->gemm_mode = mode;
  m->act_il = act_layout_interleaved();
  return sync_w_il(m);  // on the exact-fp16 path in the interleaved layout: the interleaved weight copies
}

int tvr_model_range_status(tvr_model* m, void* stream) {
  if (!m) return fail(TVR_ERR_INVALID, "tvr_model_range_status: null model");
  const hipStream_t st = (hipStream_t)stream;
  unsigned h = 0;
  TVR_HIP(hipMemcpyAsync(&h, m->range_flag, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  TVR_HIP(hipStreamSynchronize(st));
  if (h == 0) return TVR_OK;
  TVR_HIP(hipMemsetAsync(m->range_flag, 0, sizeof(unsigned), st));
  TVR_HIP(hipStreamSynchronize(st));
  return fail(TVR_ERR_RANGE, "a GEMM input reached |a| >= " + std::to_string((int)(X2_FP16_OVERFLOW / X2_ASCALE)) +
                                 ", outside the fp16-split (X2F16) range; results since the last check are not "
                                 "fp32-accurate: use gemm mode x3bf16 or f32");
}

int tvr_profile_enable(tvr_model* m, int32_t on) {
  if (!m) return fail(TVR_ERR_INVALID, "tvr_profile_enable: null model");
  TVR_HIP(hipDeviceSynchronize());
  for (auto& r : m->prof_recs) {
    m->prof_pool.push_back(r.a);
    m->prof_pool.push_back(r.b);
  }
  m->prof_recs.clear();
  m->prof = on != 0;
  return TVR_OK;
}

int tvr_profile_read(tvr_model* m, tvr_kernel_stats* out) {
  if (!m || !out) return fail(TVR_ERR_INVALID, "tvr_profile_read: null argument");
  tvr_kernel_stats s{};
  for (auto& r : m->prof_recs) {
    if (r.epi >= 3) continue;  // HBM-bound kernels: tvr_profile_read_hbm
    TVR_HIP(hipEventSynchronize(r.b));
    float ms = 0.f;
    TVR_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    s.gemm_launches[r.epi] += 1;
    s.gemm_flops[r.epi] += r.flops;
    s.gemm_bytes[r.epi] += r.bytes;
    s.gemm_ms[r.epi] += ms;
  }
  *out = s;
  return TVR_OK;
}

int tvr_profile_read_hbm(tvr_model* m, tvr_hbm_stats* out) {
  if (!m || !out) return fail(TVR_ERR_INVALID, "tvr_profile_read_hbm: null argument");
  tvr_hbm_stats s{};
  for (auto& r : m->prof_recs) {
    if (r.epi < 3) continue;
    TVR_HIP(hipEventSynchronize(r.b));
    float ms = 0.f;
    TVR_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    const int k = r.epi - 3;
    s.launches[k] += 1;
    s.ms[k] += ms;
    s.bytes[k] += r.bytes;
  }
  *out = s;
  return TVR_OK;
}

int tvr_trace_create(tvr_model* m, int32_t max_seqs, int32_t max_tokens, tvr_trace** out) {
  if (!m || !out || max_seqs <= 0 || max_tokens <= 0)
    return fail(TVR_ERR_INVALID, "tvr_trace_create: bad argument");
  const tvr_config& c = m->cfg;
  auto* t = new tvr_trace();
  t->model = m;
  t->max_seqs = max_seqs;
  t->max_tokens = max_tokens;
  const size_t per = (size_t)max_tokens * c.d_model * sizeof(float);
  hipError_t e = hipMalloc(&t->resid, per * (c.n_layers + 1));
  if (e == hipSuccess) e = hipMalloc(&t->z, per * c.n_layers);
  if (e == hipSuccess) e = hipMalloc(&t->qkv, per * 3 * c.n_layers);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    tvr_trace_destroy(t);
    return fail(TVR_ERR_NOMEM, "tvr_trace_create: device allocation failed");
  }
  *out = t;
  return TVR_OK;
}

int tvr_trace_destroy(tvr_trace* t) {
  if (!t) return TVR_OK;
  // a deferred clean forward still owes its outputs to the caller: run it once
  // everything already queued on any stream (work sharing the model's
  // workspace included) has finished, on the null stream — the deferral's
  // stream may already have been destroyed by a C caller
  int rc = TVR_OK;
  if (t->pending) {
    (void)hipDeviceSynchronize();
    rc = flush_pending(t, nullptr);
  }
  (void)hipDeviceSynchronize();
  if (t->resid) (void)hipFree(t->resid);
  if (t->z) (void)hipFree(t->z);
  if (t->qkv) (void)hipFree(t->qkv);
  delete t;
  return rc;
}

int tvr_trace_flush(tvr_trace* t, void* stream) {
  if (!t) return fail(TVR_ERR_INVALID, "tvr_trace_flush: null trace");
  return flush_pending(t, stream);
}

int tvr_trace_read(const tvr_trace* t, int32_t what, int32_t layer, float* dst, void* stream) {
  if (!t || !dst) return fail(TVR_ERR_INVALID, "tvr_trace_read: null argument");
  TVR_TRY(flush_pending(const_cast<tvr_trace*>(t), stream));  // a deferred clean forward runs now
  const int L = t->model->cfg.n_layers, d = t->model->cfg.d_model;
  const size_t stride = (size_t)t->max_tokens * d;
  const float* src = nullptr;
  if (what == TVR_TRACE_RESID_PRE && layer >= 0 && layer <= L) src = t->resid + layer * stride;
  if (what == TVR_TRACE_Z && layer >= 0 && layer < L) src = t->z + layer * stride;
  if (what >= TVR_TRACE_Q && what <= TVR_TRACE_V && layer >= 0 && layer < L) {
    // hook_q / hook_k / hook_v (before rotary): columns [(what - Q) d, .. + d) of the layer's [tokens][3 d] rows
    if (t->n_tokens > 0)
      TVR_HIP(hipMemcpy2DAsync(dst, (size_t)d * sizeof(float), t->qkv + layer * 3 * stride + (what - TVR_TRACE_Q) * d,
                               (size_t)3 * d * sizeof(float), (size_t)d * sizeof(float), (size_t)t->n_tokens,
                               hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TVR_OK;
  }
  if (!src) return fail(TVR_ERR_INVALID, "tvr_trace_read: bad hook/layer");
  if (what == TVR_TRACE_RESID_PRE && t->uncentred && t->n_tokens > 0) {
    // TL's residual stream is centred (every write to it is: W_E, W_O, W_out, their biases); the x16 path's
    // differs from it by one constant per row
    // (a caller's dst may be any float*, e.g. an offset view: the float4 form only where it is 16-B aligned)
    return launch_center_rows(src, dst, t->n_tokens, d, (hipStream_t)stream);
  }
  TVR_HIP(hipMemcpyAsync(dst, src, (size_t)t->n_tokens * d * sizeof(float), hipMemcpyDeviceToDevice,
                         (hipStream_t)stream));
  return TVR_OK;
}

int32_t tvr_trace_num_tokens(const tvr_trace* t) { return t ? t->n_tokens : 0; }

int tvr_trace_capture_resid(tvr_trace* t, const int32_t* pos, const int32_t* group, int32_t n_groups, float* out,
                            void* stream) {
  if (!t || !out) return fail(TVR_ERR_INVALID, "tvr_trace_capture_resid: null argument");
  if (t->n_seq <= 0) return fail(TVR_ERR_INVALID, "tvr_trace_capture_resid: trace is empty: run tvr_forward_clean first");
  if (n_groups <= 0) return fail(TVR_ERR_INVALID, "tvr_trace_capture_resid: n_groups must be positive");
  tvr_model* m = t->model;
  const int L = m->cfg.n_layers, d = m->cfg.d_model, n_seq = t->n_seq;
  const size_t lds = (size_t)d * sizeof(float);  // one row of sums per wave
  if (d % 4 != 0 || lds > 64 * 1024)
    return fail(TVR_ERR_UNSUPPORTED, "tvr_trace_capture_resid: d_model must be a multiple of 4, at most 16384");
  for (int s = 0; s < n_seq; ++s) {
    if (pos && (pos[s] < 0 || pos[s] >= t->seq_len[s]))
      return fail(TVR_ERR_INVALID, "tvr_trace_capture_resid: pos of sequence " + std::to_string(s) + " out of range");
    if (group && (group[s] < 0 || group[s] >= n_groups))
      return fail(TVR_ERR_INVALID, "tvr_trace_capture_resid: group of sequence " + std::to_string(s) + " out of range");
  }
  // the sequences sorted by group (stable: sequence order within a group), each group cut into chunks of
  // RESID_CAP_CHUNK rows; a group of several chunks gets consecutive partial slots and one finish item
  std::vector<int> order(n_seq);
  for (int s = 0; s < n_seq; ++s) order[s] = s;
  if (group) std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return group[a] < group[b]; });
  std::vector<int32_t> rows(n_seq);
  for (int k = 0; k < n_seq; ++k) {
    const int s = order[k];
    rows[k] = t->seq_off[s] + (pos ? pos[s] : t->seq_len[s] - 1);
  }
  std::vector<ResidCapChunk> chunks;
  std::vector<ResidCapFinish> fins;
  int n_slots = 0;
  for (int k0 = 0; k0 < n_seq;) {
    const int g = group ? group[order[k0]] : 0;
    int k1 = k0;
    while (k1 < n_seq && (group ? group[order[k1]] : 0) == g) ++k1;
    const int nch = (k1 - k0 + RESID_CAP_CHUNK - 1) / RESID_CAP_CHUNK;
    if (nch > 1) fins.push_back(ResidCapFinish{g, n_slots, nch, 0});
    for (int j = 0; j < nch; ++j) {
      const int r0 = k0 + j * RESID_CAP_CHUNK;
      chunks.push_back(ResidCapChunk{r0, std::min(RESID_CAP_CHUNK, k1 - r0), g, nch > 1 ? n_slots++ : -1});
    }
    k0 = k1;
  }
  hipStream_t st = (hipStream_t)stream;
  TVR_TRY(flush_pending(t, stream));  // a deferred clean forward runs now (it uses the workspace: carve after it)
  Carve cv;
  const size_t o_rows = cv.take<int32_t>(rows.size());
  const size_t o_chunks = cv.take<ResidCapChunk>(chunks.size());
  const size_t o_fins = cv.take<ResidCapFinish>(fins.size());
  const size_t o_part = cv.take<float>((size_t)(L + 1) * n_slots * d);
  TVR_TRY(ensure_workspace(m, cv.off, st));
  char* base = m->ws;
  UploadBatch ub;
  ub.add(o_rows, rows);
  ub.add(o_chunks, chunks);
  if (!fins.empty()) ub.add(o_fins, fins);
  TVR_TRY(flush_uploads(m, st, base, ub));
  const size_t lstride = (size_t)t->max_tokens * d;
  float* part = (float*)(base + o_part);
  ProfSpan ps(m, st);
  const dim3 g1((unsigned)chunks.size(), L + 1);
  if (t->uncentred)
    hipLaunchKernelGGL(resid_capture_partial_kernel<true>, g1, dim3(64), lds, st, t->resid, lstride,
                       (const int32_t*)(base + o_rows), (const ResidCapChunk*)(base + o_chunks), n_slots, part, out,
                       L + 1, d);
  else
    hipLaunchKernelGGL(resid_capture_partial_kernel<false>, g1, dim3(64), lds, st, t->resid, lstride,
                       (const int32_t*)(base + o_rows), (const ResidCapChunk*)(base + o_chunks), n_slots, part, out,
                       L + 1, d);
  TVR_HIP(hipGetLastError());
  if (!fins.empty()) {
    hipLaunchKernelGGL(resid_capture_finish_kernel, dim3((unsigned)fins.size(), (d + 255) / 256, L + 1), dim3(256), 0,
                       st, part, n_slots, (const ResidCapFinish*)(base + o_fins), out, L + 1, d);
    TVR_HIP(hipGetLastError());
  }
  // rows read x (L + 1) x d x 4, plus out read and written
  ps.done(TVR_HBM_CAPTURE, ((double)n_seq + 2.0 * n_groups) * (L + 1) * d * 4.0);
  return TVR_OK;
}

int tvr_trace_capture_pattern(tvr_trace* t, const int32_t* pos, const int32_t* cls, int32_t n_classes,
                              float* out_pattern, int32_t ld, float* out_mass, void* stream) {
  const char* fn = "tvr_trace_capture_pattern";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!t) return bad("null trace");
  if (t->n_seq <= 0) return bad("trace is empty: run tvr_forward_clean first");
  TVR_TRY(check_pattern_args(fn, cls, t->n_tokens, n_classes, out_pattern, out_mass));
  tvr_model* m = t->model;
  const tvr_config& c = m->cfg;
  const int L = c.n_layers, d = c.d_model, H = c.n_heads, n_seq = t->n_seq;
  std::vector<PatternSeq> seqs(n_seq);
  int max_q = 0;
  double keys = 0.0;
  for (int s = 0; s < n_seq; ++s) {
    const int q = pos ? pos[s] : t->seq_len[s] - 1;
    if (q < 0 || q >= t->seq_len[s] || q >= c.n_ctx)
      return bad("pos of sequence " + std::to_string(s) + " out of range");
    seqs[s] = PatternSeq{t->seq_off[s], q};
    max_q = std::max(max_q, q);
    keys += q + 1;
  }
  if (out_pattern && ld <= max_q) return bad("ld must exceed the largest query position (" + std::to_string(max_q) + ")");
  hipStream_t st = (hipStream_t)stream;
  TVR_TRY(flush_pending(t, stream));  // a deferred clean forward runs now (it uses the workspace: carve after it)
  Carve cv;
  const size_t o_seqs = cv.take<PatternSeq>(seqs.size());
  const size_t o_cls = out_mass ? cv.take<int32_t>((size_t)t->n_tokens) : 0;
  TVR_TRY(ensure_workspace(m, cv.off, st));
  char* base = m->ws;
  UploadBatch ub;
  ub.add(o_seqs, seqs);
  if (out_mass) ub.add(o_cls, std::vector<int32_t>(cls, cls + t->n_tokens));
  TVR_TRY(flush_uploads(m, st, base, ub));
  ProfSpan ps(m, st);
  TVR_TRY(launch_pattern(m, fn, t->qkv, (size_t)3 * t->max_tokens * d, L, (const PatternSeq*)(base + o_seqs), n_seq,
                         max_q + 1, out_mass ? (const int32_t*)(base + o_cls) : nullptr, n_classes, out_pattern, ld,
                         out_mass, nullptr, nullptr, st));
  // per layer: every sequence's Q row and its K rows [0, qpos] in, the pattern rows and the class sums out
  ps.done(TVR_HBM_ATTENTION, 4.0 * L * ((n_seq + keys) * d + (double)n_seq * H * ((out_pattern ? ld : 0) +
                                                                                   (out_mass ? n_classes : 0))));
  return TVR_OK;
}

int tvr_head_attribution(tvr_model* m, int32_t layer, const float* z, const float* dirs, int32_t n, float* out,
                         void* stream) {
  const char* fn = "tvr_head_attribution";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!m) return bad("null model");
  if (!z || !dirs || !out) return bad("null argument");
  if (n <= 0) return bad("n must be positive");
  if (layer < 0 || layer >= m->cfg.n_layers) return bad("layer out of range");
  if (((uintptr_t)z & 15) || ((uintptr_t)dirs & 15)) return bad("z and dirs must be 16-byte aligned");
  return launch_head_attribution(m, fn, dirs, n, z, 0, nullptr, layer, 1, out, (hipStream_t)stream);
}

int tvr_trace_logit_attribution(tvr_trace* t, const int32_t* pos, const int32_t* target, const int32_t* contrast,
                                float* out_head, float* out_resid, void* stream) {
  const char* fn = "tvr_trace_logit_attribution";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!t) return bad("null trace");
  if (!target) return bad("null target");
  if (!out_head && !out_resid) return bad("out_head and out_resid are both null");
  if (t->n_seq <= 0) return bad("trace is empty: run tvr_forward_clean first");
  tvr_model* m = t->model;
  const tvr_config& c = m->cfg;
  const int L = c.n_layers, d = c.d_model, n_seq = t->n_seq;
  std::vector<int32_t> rows(n_seq), tg(target, target + n_seq), ct;
  if (contrast) ct.assign(contrast, contrast + n_seq);
  for (int s = 0; s < n_seq; ++s) {
    const int q = pos ? pos[s] : t->seq_len[s] - 1;
    if (q < 0 || q >= t->seq_len[s]) return bad("pos of sequence " + std::to_string(s) + " out of range");
    if (tg[s] < 0 || tg[s] >= c.d_vocab) return bad("target of sequence " + std::to_string(s) + " outside [0, d_vocab)");
    if (contrast && (ct[s] < 0 || ct[s] >= c.d_vocab))
      return bad("contrast of sequence " + std::to_string(s) + " outside [0, d_vocab)");
    rows[s] = t->seq_off[s] + q;
  }
  if (L + 1 > 65535) return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": too many layers for one launch");
  // the direction-pass kernels read whole float4s of the trace, workspace and w_unembed_t rows
  if (d % 4 != 0 || ((uintptr_t)m->w_unembed_t & 15))
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": d_model must be a multiple of 4 and w_unembed_t 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  TVR_TRY(flush_pending(t, stream));  // a deferred clean forward runs now (it uses the workspace: carve after it)
  Carve cv;
  const size_t o_rows = cv.take<int32_t>(n_seq);
  const size_t o_tg = cv.take<int32_t>(n_seq);
  const size_t o_ct = contrast ? cv.take<int32_t>(n_seq) : 0;
  const size_t o_dirs = cv.take<float>((size_t)n_seq * d);
  TVR_TRY(ensure_workspace(m, cv.off, st));
  char* base = m->ws;
  UploadBatch ub;
  ub.add(o_rows, rows);
  ub.add(o_tg, tg);
  if (contrast) ub.add(o_ct, ct);
  TVR_TRY(flush_uploads(m, st, base, ub));
  const size_t lstride = (size_t)t->max_tokens * d;
  const int32_t* d_rows = (const int32_t*)(base + o_rows);
  float* dirs = (float*)(base + o_dirs);
  {
    ProfSpan ps(m, st);
    hipLaunchKernelGGL(attr_direction_kernel, dim3((unsigned)n_seq), dim3(64), 0, st, t->resid + L * lstride, d_rows,
                       m->w_unembed_t, (const int32_t*)(base + o_tg),
                       contrast ? (const int32_t*)(base + o_ct) : nullptr, c.ln_eps, dirs, d);
    TVR_HIP(hipGetLastError());
    if (out_resid) {
      hipLaunchKernelGGL(attr_resid_kernel, dim3((unsigned)n_seq, (unsigned)(L + 1)), dim3(64), 0, st, t->resid,
                         lstride, d_rows, dirs, out_resid, L + 1, d);
      TVR_HIP(hipGetLastError());
    }
    // the final rows and the unembed rows in, the directions out; then every layer's row and the direction in
    ps.done(TVR_HBM_CAPTURE, 4.0 * n_seq * d * ((contrast ? 4.0 : 3.0) + (out_resid ? 2.0 * (L + 1) : 0.0)));
  }
  if (out_head) TVR_TRY(launch_head_attribution(m, fn, dirs, n_seq, t->z, lstride, d_rows, 0, L, out_head, st));
  return TVR_OK;
}

int tvr_head_directions(tvr_model* m, int32_t layer, const float* dirs, int32_t n, float* out_g, void* stream) {
  const char* fn = "tvr_head_directions";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!m) return bad("null model");
  if (!dirs || !out_g) return bad("null argument");
  if (n <= 0) return bad("n must be positive");
  if (layer < 0 || layer >= m->cfg.n_layers) return bad("layer out of range");
  if (((uintptr_t)dirs & 15) || ((uintptr_t)out_g & 15)) return bad("dirs and out_g must be 16-byte aligned");
  return launch_head_directions(m, fn, dirs, n, layer, 1, out_g, (hipStream_t)stream);
}

int tvr_trace_source_attribution(tvr_trace* t, const int32_t* pos, const int32_t* target, const int32_t* contrast,
                                 const int32_t* cls, int32_t n_classes, float* out_src, int32_t ld, float* out_cls,
                                 void* stream) {
  const char* fn = "tvr_trace_source_attribution";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!t) return bad("null trace");
  if (!target) return bad("null target");
  if (t->n_seq <= 0) return bad("trace is empty: run tvr_forward_clean first");
  TVR_TRY(check_source_args(fn, cls, t->n_tokens, n_classes, out_src, out_cls));
  tvr_model* m = t->model;
  const tvr_config& c = m->cfg;
  const int L = c.n_layers, d = c.d_model, H = c.n_heads, n_seq = t->n_seq;
  std::vector<int32_t> rows(n_seq), tg(target, target + n_seq), ct;
  if (contrast) ct.assign(contrast, contrast + n_seq);
  std::vector<PatternSeq> seqs(n_seq);
  int max_q = 0;
  double keys = 0.0;
  for (int s = 0; s < n_seq; ++s) {
    const int q = pos ? pos[s] : t->seq_len[s] - 1;
    if (q < 0 || q >= t->seq_len[s] || q >= c.n_ctx)
      return bad("pos of sequence " + std::to_string(s) + " out of range");
    if (tg[s] < 0 || tg[s] >= c.d_vocab) return bad("target of sequence " + std::to_string(s) + " outside [0, d_vocab)");
    if (contrast && (ct[s] < 0 || ct[s] >= c.d_vocab))
      return bad("contrast of sequence " + std::to_string(s) + " outside [0, d_vocab)");
    rows[s] = t->seq_off[s] + q;
    seqs[s] = PatternSeq{t->seq_off[s], q};
    max_q = std::max(max_q, q);
    keys += q + 1;
  }
  if (out_src && ld <= max_q) return bad("ld must exceed the largest query position (" + std::to_string(max_q) + ")");
  // the direction kernel reads whole float4s of the trace, workspace and w_unembed_t rows
  if (d % 4 != 0 || ((uintptr_t)m->w_unembed_t & 15))
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": d_model must be a multiple of 4 and w_unembed_t 16-byte aligned");
  TVR_TRY(check_source(c, fn, n_seq, L, max_q + 1));
  // layers per group: the [layers][n_seq][d] G buffer stays within SOURCE_G_CAP_BYTES (one layer at least);
  // TVR_SOURCE_G_MB overrides the cap in MiB (read per call; 0: one layer per group; the tests compare the bits)
  const size_t g_layer = (size_t)n_seq * d;
  const size_t g_cap = (size_t)std::max(0, env_int("TVR_SOURCE_G_MB", (int)(SOURCE_G_CAP_BYTES >> 20))) << 20;
  const int per_group = (int)std::min<size_t>((size_t)L, std::max<size_t>(1, g_cap / (g_layer * sizeof(float))));
  hipStream_t st = (hipStream_t)stream;
  TVR_TRY(flush_pending(t, stream));  // a deferred clean forward runs now (it uses the workspace: carve after it)
  Carve cv;
  const size_t o_rows = cv.take<int32_t>(n_seq);
  const size_t o_tg = cv.take<int32_t>(n_seq);
  const size_t o_ct = contrast ? cv.take<int32_t>(n_seq) : 0;
  const size_t o_seqs = cv.take<PatternSeq>(seqs.size());
  const size_t o_cls = out_cls ? cv.take<int32_t>((size_t)t->n_tokens) : 0;
  const size_t o_dirs = cv.take<float>(g_layer);
  const size_t o_g = cv.take<float>(g_layer * per_group);
  TVR_TRY(ensure_workspace(m, cv.off, st));
  char* base = m->ws;
  UploadBatch ub;
  ub.add(o_rows, rows);
  ub.add(o_tg, tg);
  if (contrast) ub.add(o_ct, ct);
  ub.add(o_seqs, seqs);
  if (out_cls) ub.add(o_cls, std::vector<int32_t>(cls, cls + t->n_tokens));
  TVR_TRY(flush_uploads(m, st, base, ub));
  const size_t lstride = (size_t)t->max_tokens * d;
  float* dirs = (float*)(base + o_dirs);
  float* G = (float*)(base + o_g);
  {
    ProfSpan ps(m, st);
    hipLaunchKernelGGL(attr_direction_kernel, dim3((unsigned)n_seq), dim3(64), 0, st, t->resid + L * lstride,
                       (const int32_t*)(base + o_rows), m->w_unembed_t, (const int32_t*)(base + o_tg),
                       contrast ? (const int32_t*)(base + o_ct) : nullptr, c.ln_eps, dirs, d);
    TVR_HIP(hipGetLastError());
    // the final rows and the unembed rows in, the directions out
    ps.done(TVR_HBM_CAPTURE, 4.0 * n_seq * d * (contrast ? 4.0 : 3.0));
  }
  for (int l0 = 0; l0 < L; l0 += per_group) {
    const int nl = std::min(per_group, L - l0);
    TVR_TRY(launch_head_directions(m, fn, dirs, n_seq, l0, nl, G, st));
    ProfSpan ps(m, st);
    TVR_TRY(launch_source(m, fn, t->qkv + (size_t)l0 * 3 * lstride, 3 * lstride, nl, (const PatternSeq*)(base + o_seqs),
                          n_seq, max_q + 1, G, g_layer, out_cls ? (const int32_t*)(base + o_cls) : nullptr, n_classes,
                          out_src, ld, out_cls, l0, L, nullptr, nullptr, st));
    // per layer: every sequence's Q row, g row and its K and V rows [0, qpos] in, the source rows and class sums out
    ps.done(TVR_HBM_ATTENTION, 4.0 * nl * ((2.0 * n_seq + 2.0 * keys) * d + (double)n_seq * H * ((out_src ? ld : 0) +
                                                                                              (out_cls ? n_classes : 0))));
  }
  return TVR_OK;
}

}  // extern "C"

namespace {
// LNPre + unembed + statistics (run_final) of n rows of `x` (rows of d floats; row idx_in[i], or i when idx_in
// is empty): the workspace is carved as forward_impl carves its final stage.  targets: host [n] or null.
// run_final walks its rows in chunks through the index array (d_rows + s), so dense rows get an identity
// index, as forward_impl's all_rows path builds one: a null index is right for the first chunk only.
int decode_impl(tvr_model* m, const float* x, const std::vector<int32_t>& idx_in, int n, const int32_t* targets,
                float* out_prob, int32_t* out_topk, int topk, hipStream_t st) {
  const int d = m->cfg.d_model, fmt = act_fmt(m);
  std::vector<int32_t> idx(idx_in);
  if (idx.empty()) {
    idx.resize(n);
    for (int i = 0; i < n; ++i) idx[i] = i;
  }
  std::vector<int32_t> tg(n, -1);
  if (targets) std::copy(targets, targets + n, tg.begin());
  const int FC = std::min(final_chunk(m, fmt, nullptr), n);
  Carve cv;
  const size_t o_idx = cv.take<int32_t>(n);
  const size_t o_tg = cv.take<int32_t>(n);
  const size_t o_xf = cv.take<float>((size_t)FC * d);
  const size_t o_lg = cv.take<float>(final_scratch_floats(m, fmt, FC, topk, nullptr));
  TVR_TRY(ensure_workspace(m, cv.off, st));
  char* base = m->ws;
  UploadBatch ub;
  ub.add(o_idx, idx);
  ub.add(o_tg, tg);
  TVR_TRY(flush_uploads(m, st, base, ub));
  return run_final(m, x, (const int32_t*)(base + o_idx), (const int32_t*)(base + o_tg), n,
                   (float*)(base + o_xf), (float*)(base + o_lg), out_prob, out_topk, topk, nullptr, fmt, st);
}

// The output / top-k checks tvr_decode_rows and tvr_trace_logit_lens share; topk_eff: the k run_final gets.
int check_decode_args(const char* fn, const tvr_config& c, const int32_t* targets, int n_targets,
                      const float* out_prob, const int32_t* out_topk, int32_t topk, int& topk_eff) {
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!out_prob && !out_topk) return bad("out_prob and out_topk are both null");
  if (out_prob && !targets) return bad("out_prob needs targets");
  if (out_topk && (topk <= 0 || topk > STATS_MAX_K))
    return bad("topk must be in [1, " + std::to_string(STATS_MAX_K) + "] with out_topk");
  if (!out_topk && (topk < 0 || topk > STATS_MAX_K)) return bad("topk must be in [0, " + std::to_string(STATS_MAX_K) + "]");
  for (int i = 0; targets && i < n_targets; ++i)
    if (targets[i] < 0 || targets[i] >= c.d_vocab)
      return bad("target " + std::to_string(i) + " outside [0, d_vocab)");
  topk_eff = out_topk ? topk : 0;
  return TVR_OK;
}
}  // namespace

extern "C" {

int tvr_decode_rows(tvr_model* m, const float* rows, int32_t n, const int32_t* targets, float* out_prob,
                    int32_t* out_topk, int32_t topk, void* stream) {
  const char* fn = "tvr_decode_rows";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!m) return bad("null model");
  if (!rows) return bad("null rows");
  if (n <= 0) return bad("n must be positive");
  if ((uintptr_t)rows & 15) return bad("rows must be 16-byte aligned");
  int k = 0;
  TVR_TRY(check_decode_args(fn, m->cfg, targets, n, out_prob, out_topk, topk, k));
  return decode_impl(m, rows, {}, n, targets, out_prob, out_topk, k, (hipStream_t)stream);
}

int tvr_trace_logit_lens(tvr_trace* t, const int32_t* pos, const int32_t* targets, float* out_prob,
                         int32_t* out_topk, int32_t topk, void* stream) {
  const char* fn = "tvr_trace_logit_lens";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!t) return bad("null trace");
  if (t->n_seq <= 0) return bad("trace is empty: run tvr_forward_clean first");
  tvr_model* m = t->model;
  const int L = m->cfg.n_layers, n_seq = t->n_seq;
  int k = 0;
  TVR_TRY(check_decode_args(fn, m->cfg, targets, n_seq, out_prob, out_topk, topk, k));
  if ((int64_t)(L + 1) * t->max_tokens > INT_MAX || (int64_t)(L + 1) * n_seq > INT_MAX)
    return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": the trace's row indices do not fit in int32");
  // row l * max_tokens + row of the contiguous [L + 1][max_tokens][d] residual slabs: no copy
  std::vector<int32_t> idx((size_t)n_seq * (L + 1)), tg;
  if (targets) tg.resize(idx.size());
  for (int s = 0; s < n_seq; ++s) {
    const int q = pos ? pos[s] : t->seq_len[s] - 1;
    if (q < 0 || q >= t->seq_len[s]) return bad("pos of sequence " + std::to_string(s) + " out of range");
    for (int l = 0; l <= L; ++l) {
      idx[(size_t)s * (L + 1) + l] = l * t->max_tokens + t->seq_off[s] + q;
      if (targets) tg[(size_t)s * (L + 1) + l] = targets[s];
    }
  }
  TVR_TRY(flush_pending(t, stream));  // a deferred clean forward runs now (it uses the workspace: carve after it)
  return decode_impl(m, t->resid, idx, (int)idx.size(), targets ? tg.data() : nullptr, out_prob, out_topk, k,
                     (hipStream_t)stream);
}

}  // extern "C"

namespace {
// The checks tvr_forward_clean and its deferred form share: off[s] the first row of sequence s, R the rows.
// tokens may be null (a residual input); trace null: no capacity to check.
int check_seqs(const tvr_config& c, const tvr_trace* trace, const int32_t* tokens, const int32_t* seq_lens,
               int n_seq, std::vector<int>& off, int& R) {
  off.resize(n_seq);
  R = 0;
  for (int s = 0; s < n_seq; ++s) {
    const int T = seq_lens[s];
    if (T <= 0) return fail(TVR_ERR_INVALID, "sequence " + std::to_string(s) + " is empty");
    if (T > c.n_ctx)
      return fail(TVR_ERR_UNSUPPORTED, "sequence length " + std::to_string(T) + " exceeds n_ctx " +
                                           std::to_string(c.n_ctx));
    off[s] = R;
    R += T;
  }
  for (int r = 0; tokens && r < R; ++r)
    if (tokens[r] < 0 || tokens[r] >= c.d_vocab)
      return fail(TVR_ERR_INVALID, "token id " + std::to_string(tokens[r]) + " out of range");
  if (trace && (n_seq > trace->max_seqs || R > trace->max_tokens))
    return fail(TVR_ERR_INVALID, "trace capacity exceeded");
  return TVR_OK;
}

// The batched clean forward behind tvr_forward_clean / tvr_forward_logits.
//   tokens     host ids (embedded), or nullptr with resid_in: device [R][d]
//              hook_resid_pre of start_layer (TL forward(resid, start_at_layer=))
//   all_rows   logits of EVERY row to out_logits [R][V] (TL forward's [1, T, V]);
//              otherwise each sequence's last row (out_prob / out_topk / out_logits [n][V])
int forward_impl(tvr_model* m, tvr_trace* trace, const int32_t* tokens, const float* resid_in, int start_layer,
                 const int32_t* seq_lens, int32_t n_seq, const int32_t* targets, float* out_prob,
                 int32_t* out_topk, int32_t topk, float* out_logits, bool all_rows, float* capture_zsum,
                 void* stream) {
  if (!m || (!tokens && !resid_in) || !seq_lens || n_seq <= 0)
    return fail(TVR_ERR_INVALID, "tvr_forward_clean: bad argument");
  if (start_layer < 0 || start_layer >= m->cfg.n_layers || (tokens && start_layer != 0) || (resid_in && trace))
    return fail(TVR_ERR_INVALID, "forward: start_layer needs a residual input and no trace");
  if (topk < 0 || topk > STATS_MAX_K) return fail(TVR_ERR_INVALID, "topk must be in [0, 16]");
  if (topk > 0 && !out_topk) return fail(TVR_ERR_INVALID, "topk > 0 needs out_topk");
  hipStream_t st = (hipStream_t)stream;
  const tvr_config& c = m->cfg;
  const int d = c.d_model, L = c.n_layers;
  std::vector<int32_t> off, last(n_seq);
  int R = 0, maxT = 0;
  TVR_TRY(check_seqs(c, trace, tokens, seq_lens, n_seq, off, R));
  for (int s = 0; s < n_seq; ++s) {
    last[s] = off[s] + seq_lens[s] - 1;
    maxT = std::max(maxT, seq_lens[s]);
  }
  if (trace) trace->uncentred = use_x16(m);

  std::vector<SeqDesc> seqs(n_seq);
  for (int s = 0; s < n_seq; ++s) seqs[s] = {off[s], seq_lens[s], 0, -1, 0, 0};
  std::vector<int32_t> tok = tokens ? std::vector<int32_t>(tokens, tokens + R) : std::vector<int32_t>();
  // Shared prefixes without a trace (only each prompt's last row is read
  // afterwards): a prompt whose leading tokens equal those of the first prompt
  // with its first token computes only the rows after the common prefix and
  // reads the prefix K/V from that prompt's rows (SeqDesc.prefix_live); every
  // extraction prompt starts with BOS.  With a trace every row is kept (patch
  // sweeps read any position of it).
  if (!trace && tokens && !all_rows && prefix_share_enabled()) {
    std::map<int, int> first;  // first token -> first prompt starting with it
    std::vector<int32_t> ctok;
    ctok.reserve(R);
    int Rc = 0;
    for (int s = 0; s < n_seq; ++s) {
      const int T = seq_lens[s];
      const int32_t* tk = tokens + off[s];
      const int ld = first.emplace(tk[0], s).first->second;  // (s itself: the first prompt with this token)
      const int P = ld == s ? 0 : shared_prefix_len(tk, T, tokens + off[ld], seq_lens[ld]);
      seqs[s] = P > 0 ? SeqDesc{Rc, T - P, P, seqs[ld].row0, 0, 1} : SeqDesc{Rc, T, 0, -1, 0, 0};
      ctok.insert(ctok.end(), tk + P, tk + T);
      last[s] = Rc + T - P - 1;
      Rc += T - P;
    }
    tok.swap(ctok);
    R = Rc;
  }
  // without a trace only each prompt's last row is read after the last layer
  const bool trim = trace == nullptr && !all_rows;
  std::vector<SeqDesc> seqs_last(seqs);
  for (auto& q : seqs_last) q.q0 = q.n - 1;
  std::vector<int32_t> tg(n_seq, -1);
  if (targets) std::copy(targets, targets + n_seq, tg.begin());

  const int n_out = all_rows ? R : n_seq;  // rows of the final LN + unembed
  std::vector<int32_t> out_rows;
  if (all_rows) {
    out_rows.resize(R);
    for (int r = 0; r < R; ++r) out_rows[r] = r;
  }
  const int FC = std::min(final_chunk(m, act_fmt(m), out_logits), n_out);
  Carve cv;
  const size_t o_seqs = cv.take<SeqDesc>(n_seq);
  const size_t o_seqs_last = cv.take<SeqDesc>(n_seq);
  const size_t o_tok = cv.take<int32_t>(R);
  const size_t o_last = cv.take<int32_t>(n_seq);
  const size_t o_rows = all_rows ? cv.take<int32_t>(R) : 0;
  const size_t o_tg = cv.take<int32_t>(n_seq);
  const size_t o_resid = cv.take<float>((size_t)R * d);
  const size_t o_xn = cv.take<float>((size_t)R * d);
  const size_t o_xn2 = use_x16(m) ? cv.take<float>((size_t)R * d) : 0;
  const size_t o_qkv = trace ? 0 : cv.take<float>((size_t)R * 3 * d);
  const size_t o_a2 = cv.take<float>((size_t)R * m->K2);
  const size_t o_xf = cv.take<float>((size_t)FC * d);
  const size_t o_lg = cv.take<float>(final_scratch_floats(m, act_fmt(m), FC, topk, out_logits));
  const int n_cap = capture_zsum ? L - start_layer : 0;  // layers captured (one reduction after the loop)
  const size_t o_cap = capture_zsum ? cv.take<float>((size_t)n_cap * CAP_GROUPS * d) : 0;
  // fp32 hook_z of each prompt's last row, every layer, for the capture when no
  // trace slot receives it (the attention kernel writes that row only, at row s
  // of the layer's slab)
  const bool zf_last = capture_zsum && !trace;
  const size_t o_zf = zf_last ? cv.take<float>((size_t)n_cap * n_seq * d) : 0;
  TVR_TRY(ensure_workspace(m, cv.off, st));
  char* base = m->ws;
  UploadBatch ub;
  ub.add(o_seqs, seqs);
  ub.add(o_seqs_last, seqs_last);
  ub.add(o_tok, tok);
  ub.add(o_last, last);
  if (all_rows) ub.add(o_rows, out_rows);
  ub.add(o_tg, tg);
  TVR_TRY(flush_uploads(m, st, base, ub));

  const int fmt = act_fmt(m);
  Acts a{(float*)(base + o_resid), (float*)(base + o_xn), trace ? nullptr : (float*)(base + o_qkv),
         (float*)(base + o_a2), acts_fmt(m)};
  if (use_x16(m)) a.xn2 = (float*)(base + o_xn2);
  const SeqDesc* d_seqs = (const SeqDesc*)(base + o_seqs);
  const int32_t* d_last = (const int32_t*)(base + o_last);
  const size_t tstride = trace ? (size_t)trace->max_tokens * d : 0;

  if (tokens) {
    const size_t total = (size_t)R * (d / 4);
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(embed_kernel, dim3(blocks), dim3(256), 0, st, (const int32_t*)(base + o_tok),
                       m->w_embed, a.resid, R, d);
    TVR_HIP(hipGetLastError());
  } else {
    TVR_HIP(hipMemcpyAsync(a.resid, resid_in, (size_t)R * d * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  for (int l = start_layer; l < L; ++l) {
    if (trace)
      TVR_HIP(hipMemcpyAsync(trace->resid + l * tstride, a.resid, (size_t)R * d * sizeof(float),
                             hipMemcpyDeviceToDevice, st));
    float* qkv = trace ? trace->qkv + (size_t)l * 3 * tstride : a.qkv;
    // attention writes the fp32 hook_z straight into the trace (or the capture buffer)
    float* zf = trace ? trace->z + l * tstride
                      : (capture_zsum ? (float*)(base + o_zf) + (size_t)(l - start_layer) * n_seq * d : nullptr);
    const bool want_out = out_prob || out_topk || out_logits;
    if (trim && l == L - 1) {
      TVR_TRY(run_block_last_rows(m, l, R, (const SeqDesc*)(base + o_seqs_last), n_seq, maxT, a, nullptr,
                                  d_last, n_seq, want_out, zf, st, zf_last));
    } else {
      TVR_TRY(run_block(m, l, R, d_seqs, n_seq, maxT, a, qkv, nullptr, zf, st, zf_last));
    }
    if (!(trim && l == L - 1)) TVR_TRY(run_block_out(m, l, R, a, st));
  }
  if (capture_zsum) {  // every layer's Σ over prompts of hook_z at the last row: one launch pair
    float* part = (float*)(base + o_cap);
    const float* z0 = trace ? trace->z + start_layer * tstride : (const float*)(base + o_zf);
    ProfSpan ps(m, st);
    hipLaunchKernelGGL(capture_partial_kernel, dim3((d / 4 + 63) / 64, CAP_GROUPS, n_cap), dim3(64), 0, st,
                       z0, d, trace ? tstride : (size_t)n_seq * d, zf_last ? nullptr : d_last, n_seq, part, d);
    hipLaunchKernelGGL(capture_finish_kernel, dim3((d + 255) / 256, n_cap), dim3(256), 0, st, part,
                       capture_zsum + (size_t)start_layer * d, d);
    TVR_HIP(hipGetLastError());
    ps.done(TVR_HBM_CAPTURE, (double)n_cap * ((double)n_seq + 1.0) * d * 4.0);  // hook_z at every last row in, [L][d] out
  }
  if (trace) {
    TVR_HIP(hipMemcpyAsync(trace->resid + L * tstride, a.resid, (size_t)R * d * sizeof(float),
                           hipMemcpyDeviceToDevice, st));
    trace->seq_off.assign(off.begin(), off.end());
    trace->seq_len.assign(seq_lens, seq_lens + n_seq);
    trace->tokens.assign(tokens, tokens + R);  // trace => tokens (checked above)
    trace->n_seq = n_seq;
    trace->n_tokens = R;
  }
  if (all_rows)
    TVR_TRY(run_final(m, a.resid, (const int32_t*)(base + o_rows), nullptr, R, (float*)(base + o_xf),
                      (float*)(base + o_lg), nullptr, nullptr, 0, out_logits, fmt, st));
  else if (out_prob || out_topk || out_logits)
    TVR_TRY(run_final(m, a.resid, d_last, (const int32_t*)(base + o_tg), n_seq, (float*)(base + o_xf),
                      (float*)(base + o_lg), out_prob, out_topk, topk, out_logits, fmt, st));
  return TVR_OK;
}
// Run a deferred clean forward on its own (the trace is used other than by a
// patch sweep).
int flush_pending(tvr_trace* t, void* stream) {
  if (!t->pending) return TVR_OK;
  t->pending = false;
  const std::vector<int32_t> tok(t->tokens), lens(t->seq_len), tg(t->p_targets);
  return forward_impl(t->model, t, tok.data(), nullptr, 0, lens.data(), (int32_t)lens.size(),
                      tg.empty() ? nullptr : tg.data(), t->p_prob, t->p_topk, t->p_k, nullptr, false, nullptr, stream);
}
}  // namespace

extern "C" {

int tvr_forward_clean(tvr_model* m, tvr_trace* trace, const int32_t* tokens, const int32_t* seq_lens,
                      int32_t n_seq, const int32_t* targets, float* out_prob, int32_t* out_topk,
                      int32_t topk, float* out_logits, float* capture_zsum, void* stream) {
  if (!tokens) return fail(TVR_ERR_INVALID, "tvr_forward_clean: bad argument");
  if (trace) TVR_TRY(flush_pending(trace, stream));  // its outputs are owed to the caller
  return forward_impl(m, trace, tokens, nullptr, 0, seq_lens, n_seq, targets, out_prob, out_topk, topk, out_logits,
                      false, capture_zsum, stream);
}

int tvr_forward_clean_deferred(tvr_model* m, tvr_trace* trace, const int32_t* tokens, const int32_t* seq_lens,
                               int32_t n_seq, const int32_t* targets, float* out_prob, int32_t* out_topk,
                               int32_t topk, void* stream) {
  if (!m || !trace || !tokens || !seq_lens || n_seq <= 0)
    return fail(TVR_ERR_INVALID, "tvr_forward_clean_deferred: bad argument");
  if (trace->model != m) return fail(TVR_ERR_INVALID, "trace belongs to another model");
  if (topk < 0 || topk > STATS_MAX_K) return fail(TVR_ERR_INVALID, "topk must be in [0, 16]");
  if (topk > 0 && !out_topk) return fail(TVR_ERR_INVALID, "topk > 0 needs out_topk");
  TVR_TRY(flush_pending(trace, stream));
  std::vector<int> off;
  int R = 0;
  TVR_TRY(check_seqs(m->cfg, trace, tokens, seq_lens, n_seq, off, R));
  trace->seq_off = off;
  trace->seq_len.assign(seq_lens, seq_lens + n_seq);
  trace->tokens.assign(tokens, tokens + R);
  trace->n_seq = n_seq;
  trace->n_tokens = R;
  trace->p_targets = targets ? std::vector<int32_t>(targets, targets + n_seq) : std::vector<int32_t>();
  trace->p_prob = out_prob;
  trace->p_topk = out_topk;
  trace->p_k = topk;
  trace->p_stream = stream;
  trace->pending = true;
  return TVR_OK;
}

int tvr_forward_logits(tvr_model* m, const int32_t* tokens, const float* resid_in, int32_t start_layer,
                       const int32_t* seq_lens, int32_t n_seq, float* out_logits, void* stream) {
  if (!out_logits || (tokens == nullptr) == (resid_in == nullptr))
    return fail(TVR_ERR_INVALID, "tvr_forward_logits: give exactly one of tokens / resid_in, and out_logits");
  return forward_impl(m, nullptr, tokens, resid_in, start_layer, seq_lens, n_seq, nullptr, nullptr, nullptr, 0,
                      out_logits, true, nullptr, stream);
}



// What the sweep's per-layer launches read: the plan, its tables in the workspace and the lin-entry scratch.
struct SweepCtx {
  tvr_model* m;
  tvr_trace* trace;
  const SweepPlan& p;
  bool fused;
  Acts& a;
  const float* vectors;
  hipStream_t st;
  const SeqDesc* seqs;
  const EntryDesc* ents;
  const int32_t* egidx;
  const EntryGroup* egroups;
  const LinRow* lin_rows;
  const LinMB* lin_mbs;
  const int32_t* lin_vids;
  float2* lnstats;
  float* raw_h;
  uint16_t* vact;  // vectors in the activation format
  float* g;
  uint16_t* vg;  // exact-fp16 weights: one layer's G rows (centred vectors x LN1 / LN2 gamma, activation format)
};

// The sites entering at layer l (L: the final norm's input) materialise their residual rows.  resid_base / z_base:
// the clean hook_resid_pre [L + 1] and attn.hook_z [L] planes, tstride floats apart (the trace's; tvr_site_entry:
// a caller's).  force_valu (tvr_site_entry only): REPLACE_HEAD sites take entry_kernel's own branch.
static int sweep_enter(const SweepCtx& cx, int l, const float* resid_base, const float* z_base, size_t tstride,
                       bool force_valu = false) {
  tvr_model* m = cx.m;
  const SweepPlan& p = cx.p;
  const tvr_config& c = m->cfg;
  const int d = c.d_model, k0 = l > 0 ? p.cnt_le[l - 1] : 0, k1 = p.cnt_le[l];
  if (k1 <= k0) return TVR_OK;
  // the clean rows' hook_resid_pre: the live rows [0, Rc) in a fused sweep (the trace's copy is written by
  // this layer's LayerNorm, after the entry), else the trace
  const float* snap = cx.fused ? cx.a.resid : resid_base + (size_t)l * tstride;
  const float* zsnap = l > 0 ? z_base + (size_t)(l - 1) * tstride : nullptr;
  const float* w2 = l > 0 ? m->layers[l - 1].w2 : nullptr;
  const dim3 eg(k1 - k0, (d + ENTRY_THREADS - 1) / ENTRY_THREADS);
  ProfSpan ps(m, cx.st);
  const bool mf = !force_valu && p.eg_cnt[l] > 0 &&
                  (c.d_head == 16 || c.d_head == 64 || c.d_head == 80 || c.d_head == 128);
  if (mf) {
    const dim3 gg(p.eg_cnt[l], (d + ENTRY_COLS - 1) / ENTRY_COLS);
#define TVR_ENTRY_MF(DH)                                                                                     \
  hipLaunchKernelGGL(entry_replace_mfma_kernel<DH>, gg, dim3(ENTRY_THREADS), 0, cx.st, cx.ents, cx.egidx,     \
                     cx.egroups + p.eg_beg[l], snap, zsnap, w2, m->K2, cx.vectors, cx.a.resid, d)
    switch (c.d_head) {
      case 16: TVR_ENTRY_MF(16); break;
      case 64: TVR_ENTRY_MF(64); break;
      case 80: TVR_ENTRY_MF(80); break;
      default: TVR_ENTRY_MF(128); break;
    }
#undef TVR_ENTRY_MF
    TVR_HIP(hipGetLastError());
  }
  if (p.ent_other[l] || !mf) {
    const size_t zbytes = mf ? 0 : (size_t)std::min(p.maxT, ENTRY_LDS_POS) * c.d_head * sizeof(float);
    if (zbytes > 64 * 1024)
      TVR_HIP(hipFuncSetAttribute((const void*)entry_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)zbytes));
    hipLaunchKernelGGL(entry_kernel, eg, dim3(ENTRY_THREADS), zbytes, cx.st, cx.ents + k0, snap, zsnap, w2, m->K2,
                       cx.vectors, cx.a.resid, d, c.d_head, mf ? 1 : 0);
    TVR_HIP(hipGetLastError());
  }
  ps.done(TVR_HBM_ENTRY, p.entry_bytes[l]);
  return TVR_OK;
}

// Layer l's block with the linearised entry rows [Rp, Rl) (p.use_lin[l])
static int sweep_block_lin(const SweepCtx& cx, int l, int Rl, const float* cache, float* zf) {
  tvr_model* m = cx.m;
  const SweepPlan& p = cx.p;
  Acts& a = cx.a;
  hipStream_t st = cx.st;
  const tvr_config& c = m->cfg;
  const tvr_layer_weights& w = m->layers[l];
  const int d = c.d_model, fmt = act_fmt(m), Rc = p.Rc, Rp = Rc + p.rows_le[l - 1], D1 = m->D1, nv = p.lin_nv[l];
  const int32_t* vids = cx.lin_vids + p.lin_vid_off[l];
  TVR_TRY(launch_lnpre(a.resid, d, nullptr, a.xn, d, Rl, d, c.ln_eps, a.fmt, st, m, cx.lnstats, a.resid_mirror,
                       a.mirror_rows, a.xn2 ? m->g1[l] : nullptr, a.xn2 ? m->g2[l] : nullptr, a.xn2));
  GemmEpi e1 = epi_qkv_mlpin(m, w.b1, a.qkv, a);
  e1.raw = cx.raw_h;
  e1.raw_rows = Rc;
  e1.ld_raw = c.d_mlp;
  TVR_TRY(launch_w1(m, l, a.xn, Rp, 0, D1, e1, st, a.xn2));
  ProfSpan ps(m, st);
  const bool prof = m->prof;
  m->prof = false;  // G and the entry rows are timed as one HBM-kind span, not as GEMM-family launches
  GemmEpi eg{};
  eg.out0 = cx.g;
  eg.ld0 = D1;
  eg.a_rows = vids;
  eg.skinny = 1;
  int rc = TVR_OK;
  const int nqk = fmt == ACT_BF16 && !m->w1qk.empty() ? 2 * d : 0;  // bf16: Q / K columns on fp16 operands
  if (use_x16(m)) {
    // G = v W1'^T on the raw fp16 W1 (one plane, 2 products): rows ((v - mean) o gamma1 | gamma2), lin_entry.hpp
    uint16_t* vg1 = cx.vg;
    uint16_t* vg2 = vg1 + (size_t)2 * nv * d;
    hipLaunchKernelGGL(lin_gamma_rows_kernel, dim3((nv + 3) / 4), dim3(256), 0, st, cx.vectors, d, vids, m->g1[l],
                       m->g2[l], vg1, vg2, nv, m->range_flag);
    rc = hipGetLastError() == hipSuccess ? TVR_OK : fail(TVR_ERR_HIP, "lin_gamma_rows_kernel launch");
    GemmEpi ex = eg;
    ex.a_rows = nullptr;  // the rows are the layer's vectors in order
    const int q = 3 * d;  // first MLP-in column: it and the columns after it read the gamma2 rows
    if (rc == TVR_OK && q % 256 == 0) {
      ex.a2 = vg2;
      ex.a2_col = q;
      rc = launch_gemm(EPI_BIAS, vg1, d, fmt, m->w1x[l], d, nv, D1, d, ex, st, m);
    } else if (rc == TVR_OK) {  // two launches (d % 256 != 0: the tiny test model)
      rc = launch_gemm(EPI_BIAS, vg1, d, fmt, m->w1x[l], d, nv, q, d, ex, st, m);
      GemmEpi e2 = ex;
      e2.out0 = ex.out0 + q;
      MatW Wq;
      if (rc == TVR_OK) rc = w_from_row(m->w1x[l], q, d, Wq);
      if (rc == TVR_OK) rc = launch_gemm(EPI_BIAS, vg2, d, fmt, Wq, d, nv, D1 - q, d, e2, st, m);
    }
  } else if (nqk > 0) {
    rc = launch_gemm(EPI_BIAS, cx.vact + d, d, ACT_F16, m->w1qk[l], d, nv, nqk, d, eg, st, m);
    GemmEpi e2 = eg;
    e2.out0 = eg.out0 + nqk;
    if (rc == TVR_OK)
      rc = launch_gemm(EPI_BIAS, cx.vact, d, fmt, m->w1[l].rows((size_t)nqk * d), d, nv, D1 - nqk, d, e2, st, m);
  } else {
    rc = launch_gemm(EPI_BIAS, cx.vact, d, fmt, m->w1[l], d, nv, D1, d, eg, st, m);
  }
  m->prof = prof;
  TVR_TRY(rc);
  const int npl = fmt == ACT_X2F16 ? 2 : 1, KP = m->lin_kp, nmb = p.lin_nmb[l];
  const size_t per = (size_t)c.n_heads * D1 * KP;
  const uint16_t* wp = m->lin_planes + (size_t)(l - 1) * npl * per;
  // X2F16: every column tile in one launch; BF16: the Q / K column tiles [0, 2d) on the fp16 rows of the
  // planes (scale lin_scale[l]), the rest on bf16
  const int n_ct = (D1 + 255) / 256, ct_qk = fmt == ACT_BF16 ? lin_qk_cols(c) / 256 : 0;
  float acc_scale = fmt == ACT_X2F16 ? 1.0f / (m->lin_scale[l] * X2_ASCALE) : 1.0f;
  dim3 g;
  int ct_base = 0;
#define TVR_LIN(F, NK, ...)                                                                                          \
  hipLaunchKernelGGL((lin_entry_kernel<F, NK __VA_OPT__(,) __VA_ARGS__>), g, dim3(LIN_THREADS), 0, st,                \
                     cx.lin_mbs + p.lin_mb_off[l], nmb, cx.lin_rows, wp, per, acc_scale,                              \
                     cx.trace->z + (size_t)(l - 1) * cx.trace->max_tokens * d, d, c.d_head, cx.lnstats, a.qkv,        \
                     cx.raw_h, c.d_mlp, cx.g, m->lin_c1 + (size_t)l * D1, w.b1, D1,                                   \
                     reinterpret_cast<uint16_t*>(a.a2) + act_col_rt(a.fmt, d), 2 * m->K2, m->K2, m->range_flag, ct_base)
#define TVR_LIN_K(F, ...)                                                 \
  if (KP == 32) TVR_LIN(F, 1 __VA_OPT__(,) __VA_ARGS__);                  \
  else if (KP == 64) TVR_LIN(F, 2 __VA_OPT__(,) __VA_ARGS__);             \
  else if (KP == 96) TVR_LIN(F, 3 __VA_OPT__(,) __VA_ARGS__);             \
  else TVR_LIN(F, 4 __VA_OPT__(,) __VA_ARGS__)
  if (fmt == ACT_X2F16 && a.fmt == ACT_X2F16I) {  // a2's GELU planes interleaved
    g = dim3(nmb * n_ct);
    TVR_LIN_K(ACT_X2F16, true);
  } else if (fmt == ACT_X2F16) {
    g = dim3(nmb * n_ct);
    TVR_LIN_K(ACT_X2F16);
  } else {
    if (ct_qk > 0) {
      g = dim3(nmb * ct_qk);
      acc_scale = 1.0f / m->lin_scale[l];
      TVR_LIN_K(ACT_F16);
    }
    g = dim3(nmb * (n_ct - ct_qk));
    acc_scale = 1.0f;
    ct_base = ct_qk;
    TVR_LIN_K(ACT_BF16);
  }
#undef TVR_LIN_K
#undef TVR_LIN
  TVR_HIP(hipGetLastError());
  // algorithmic bytes: the entering rows' outputs written and their clean rows' y_c read (4 B per
  // column each), z slices, the layer's Wsc planes once, G written + read, the vectors' planes
  ps.done(TVR_HBM_LIN_ENTRY, (double)p.lin_nrows[l] * (8.0 * D1 + 4.0 * c.d_head) + 2.0 * npl * per +
                                 nv * (8.0 * D1 + 4.0 * d) + 2.0 * npl * (double)D1 * d);
  ProfSpan pa(m, st);
  TVR_TRY(launch_attention(m, a.qkv, cache, cx.seqs, p.nc + p.cnt_le[l], p.maxT, a.a2, a.fmt, zf, st, false, Rc));
  pa.done(TVR_HBM_ATTENTION, attention_bytes(d, Rl, Rl, a.fmt, zf ? std::min(Rl, Rc) : 0));
  return run_block_out(m, l, Rl, a, st);
}

// The body of tvr_patch_sweep and tvr_patch_sweep_sets.  set_off == nullptr: the plain sweep (kinds 0-3
// and 6 only); else sites of kinds 4 / 5 own patches[set_off[i], set_off[i + 1]) and the other kinds own nothing.
// Without set sites every head-set table is empty and no launch is added.  key_off != nullptr
// (tvr_patch_sweep_knockout, with set_off): sites of kind 7 own patches as their members and
// keys[key_off[i], key_off[i + 1]); without such sites the knockout tables are empty and no launch is added.
static int sweep_impl(const char* fn, tvr_model* m, tvr_trace* trace, const tvr_site* sites, int32_t n_sites,
                      const int32_t* set_off, const tvr_head_patch* patches, const int32_t* key_off,
                      const int32_t* keys, const float* vectors,
                      int32_t n_vectors, float* out_prob, int32_t* out_topk, int32_t topk, float* out_logits,
                      void* stream) {
  if (!m || !trace || !sites || n_sites <= 0)
    return fail(TVR_ERR_INVALID, std::string(fn) + ": bad argument");
  if (trace->model != m) return fail(TVR_ERR_INVALID, "trace belongs to another model");
  if (trace->n_seq <= 0) return fail(TVR_ERR_INVALID, "trace is empty: run tvr_forward_clean first");
  if (topk < 0 || topk > STATS_MAX_K) return fail(TVR_ERR_INVALID, "topk must be in [0, 16]");
  if (topk > 0 && !out_topk) return fail(TVR_ERR_INVALID, "topk > 0 needs out_topk");
  hipStream_t st = (hipStream_t)stream;
  const tvr_config& c = m->cfg;
  const int d = c.d_model, L = c.n_layers, fmt = act_fmt(m);
  // Fused clean forward (a deferred tvr_forward_clean on this trace): the
  // clean rows [0, Rc) (trace row layout) run in the same launches as the
  // site rows, which follow them; the sites read the clean K/V from the live
  // buffer, and the trace is filled as the layers go.  This removes the clean
  // forward's own small-M launches (52 prompts x 3 tokens).
  const bool fused = trace->pending;
  if (fused) trace->uncentred = use_x16(m);  // this sweep fills the trace's clean rows

  // --- plan (sweep_plan.hpp) ------------------------------------------------
  const SweepPlanIn in{L, c.n_heads, d, c.d_head, trace->seq_off.data(), trace->seq_len.data(),
                       trace->tokens.data(), trace->n_seq, trace->n_tokens, fused,
                       prefix_share_enabled() && (int)trace->tokens.size() >= trace->n_tokens,
                       fused && fmt != ACT_F32 && L >= 3 && lin_entry_enabled(), ENTRY_GROUP, n_vectors,
                       vectors != nullptr, ((uintptr_t)vectors & 15) == 0, fmt == ACT_BF16 ? 2.0 : 4.0,
                       sites, n_sites, set_off, patches, key_off, keys};
  SweepPlan p;
  std::string err;
  const int prc = plan_sweep(in, p, err);
  if (prc != TVR_OK) return fail(prc, err);
  if (!p.ko_items.empty()) TVR_TRY(check_knockout(c, fn, *std::max_element(p.ko_max_keys.begin(), p.ko_max_keys.end())));
  const int Rc = p.Rc, nc = p.nc;
  bool any_lin = !p.lin_mbs.empty();
  if (any_lin) {
    const int rc = ensure_lin(m, st);
    if (rc == TVR_ERR_NOMEM) {  // the W1 W_O planes do not fit: the full-GEMM entry (TVR_LIN_ENTRY=0) instead
      any_lin = false;
      p.drop_lin();
    } else {
      TVR_TRY(rc);
    }
  }
  std::vector<int32_t> clean_tg(nc, -1);
  if (fused && !trace->p_targets.empty()) clean_tg = trace->p_targets;
  const int ktop = std::max(topk, fused ? trace->p_k : 0);

  // --- workspace and tables ---------------------------------------------------
  const int RA = Rc + p.R;  // rows of the activation buffers
  // run_final chunks: the sites' (logits requested or not) and the fused clean rows' (never logits)
  const int FCs = std::min(final_chunk(m, fmt, out_logits), n_sites), FCc = std::min(final_chunk(m, fmt, nullptr), nc);
  Carve cv;
  UploadBatch ub;
  // the uploaded tables first, carved in this order: flush_uploads sends one span from the first to the last
  // (the clean tables are empty unless fused, the lin tables without lin layers, the head-set tables without sets)
  auto table = [&](const auto& v) {
    const size_t at = cv.take<typename std::decay_t<decltype(v)>::value_type>(v.size());
    ub.add(at, v);
    return at;
  };
  const size_t o_seqs = table(p.seqs);
  const size_t o_seqs_last = table(p.seqs_last);
  const size_t o_last_sorted = table(p.last_sorted);
  const size_t o_ents = table(p.ents);
  const size_t o_last = table(p.last);
  const size_t o_tg = table(p.tg);
  const size_t o_clast = table(p.clean_last);
  const size_t o_ctg = table(clean_tg);
  const size_t o_ctok = table(std::vector<int32_t>(trace->tokens.begin(), trace->tokens.begin() + Rc));
  const size_t o_lin_rows = table(p.lin_rows);
  const size_t o_lin_mbs = table(p.lin_mbs);
  const size_t o_lin_vids = table(p.lin_vids);
  const size_t o_egidx = table(p.egidx);
  const size_t o_egroups = table(p.egroups);
  const size_t o_hs_items = table(p.hs_items);
  const size_t o_hs_patches = table(p.hs_patches);
  const size_t o_ko_items = table(p.ko_items);
  const size_t o_ko_masks = table(p.ko_masks);
  const size_t o_resid = cv.take<float>((size_t)RA * d);
  const size_t o_xn = cv.take<float>((size_t)RA * d);
  const size_t o_xn2 = use_x16(m) ? cv.take<float>((size_t)RA * d) : 0;
  const size_t o_qkv = cv.take<float>((size_t)RA * 3 * d);
  const size_t o_a2 = cv.take<float>((size_t)RA * m->K2);
  const size_t o_xf = cv.take<float>((size_t)std::max(FCs, FCc) * d);
  const size_t o_lg = cv.take<float>(std::max(final_scratch_floats(m, fmt, FCs, ktop, out_logits),
                                              final_scratch_floats(m, fmt, FCc, ktop, nullptr)));
  const size_t o_lnstats = cv.take<float2>(any_lin ? RA : 0);
  const size_t o_raw = cv.take<float>(any_lin ? (size_t)Rc * c.d_mlp : 0);
  const size_t o_vact = cv.take<float>(any_lin ? (size_t)n_vectors * d : 0);
  const size_t o_g = cv.take<float>((size_t)p.lin_max_nv * m->D1);
  const size_t o_vg = cv.take<float>(any_lin && use_x16(m) ? (size_t)2 * p.lin_max_nv * d : 0);
  TVR_TRY(ensure_workspace(m, cv.off, st));
  char* base = m->ws;
  TVR_TRY(flush_uploads(m, st, base, ub));

  // --- run --------------------------------------------------------------------
  Acts a{(float*)(base + o_resid), (float*)(base + o_xn), (float*)(base + o_qkv),
         (float*)(base + o_a2), acts_fmt(m)};
  if (use_x16(m)) a.xn2 = (float*)(base + o_xn2);
  const SweepCtx cx{m, trace, p, fused, a, vectors, st, (const SeqDesc*)(base + o_seqs),
                    (const EntryDesc*)(base + o_ents), (const int32_t*)(base + o_egidx),
                    (const EntryGroup*)(base + o_egroups), (const LinRow*)(base + o_lin_rows),
                    (const LinMB*)(base + o_lin_mbs), (const int32_t*)(base + o_lin_vids),
                    (float2*)(base + o_lnstats), (float*)(base + o_raw), (uint16_t*)(base + o_vact),
                    (float*)(base + o_g), (uint16_t*)(base + o_vg)};
  const size_t tstride = (size_t)trace->max_tokens * d;
  if (fused) {
    const size_t total = (size_t)Rc * (d / 4);
    hipLaunchKernelGGL(embed_kernel, dim3((int)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0, st,
                       (const int32_t*)(base + o_ctok), m->w_embed, a.resid, Rc, d);
    TVR_HIP(hipGetLastError());
  }
  if (any_lin) {
    const size_t n = (size_t)n_vectors * d;
    const dim3 g((unsigned)std::min<size_t>((n + 255) / 256, 8192));
    if (fmt == ACT_X2F16)
      hipLaunchKernelGGL(act_rows_kernel<ACT_X2F16>, g, dim3(256), 0, st, vectors, d, cx.vact, n_vectors, d,
                         m->range_flag);
    else  // bf16 plane + the fp16 plane the Q / K columns of G read (as LayerNorm's store_ln4)
      hipLaunchKernelGGL(act_rows_bf16_f16_kernel, g, dim3(256), 0, st, vectors, d, cx.vact, n_vectors, d);
    TVR_HIP(hipGetLastError());
  }
  for (int l = 0; l < L; ++l) {
    const int Rl = Rc + p.rows_le[l];
    float* tqkv = trace->qkv + (size_t)l * 3 * tstride;
    if (fused) {  // the clean rows' hook_resid_pre / K,V cache go to the trace from the kernels writing them
      a.resid_mirror = trace->resid + l * tstride;
      a.qkv_mirror = tqkv;
      a.mirror_rows = Rc;
    }
    TVR_TRY(sweep_enter(cx, l, trace->resid, trace->z, tstride));
    if (Rl == 0) continue;
    a.hs_n = p.hs_beg[l + 1] - p.hs_beg[l];  // this layer's head-set patches (0 without set sites)
    if (a.hs_n > 0) {
      a.hs_items = (const HeadsetItem*)(base + o_hs_items) + p.hs_beg[l];
      a.hs_patches = (const HeadsetPatch*)(base + o_hs_patches);
      a.hs_vectors = vectors;
      a.hs_max_rows = p.hs_max_rows[l];
      a.hs_bytes = p.hs_bytes[l];
    }
    const float* cache = fused ? a.qkv : tqkv;
    a.ko_n = p.ko_beg[l + 1] - p.ko_beg[l];  // this layer's attention knockouts (0 without kind-7 sites)
    if (a.ko_n > 0) {
      a.ko_items = (const KnockoutItem*)(base + o_ko_items) + p.ko_beg[l];
      a.ko_masks = (const uint32_t*)(base + o_ko_masks);
      a.ko_seqs = cx.seqs;  // (the last layer's table differs in q0 only, which the kernel does not read)
      a.ko_cache = cache;
      a.ko_max_keys = p.ko_max_keys[l];
      a.ko_bytes = p.ko_bytes[l];
    }
    float* zf = fused ? trace->z + l * tstride : nullptr;  // the clean rows' hook_z (rows < Rc)
    if (p.use_lin[l]) {
      TVR_TRY(sweep_block_lin(cx, l, Rl, cache, zf));
    } else if (l == L - 1 && Rc + p.cnt_le[l] < Rl) {  // (every row a last row, e.g. C2's: the plain block)
      TVR_TRY(run_block_last_rows(m, l, Rl, (const SeqDesc*)(base + o_seqs_last), nc + p.cnt_le[l], p.maxT, a, cache,
                                  (const int32_t*)(base + o_last_sorted), Rc + p.cnt_le[l], true, zf, st, false, Rc,
                                  nc));
    } else {
      TVR_TRY(run_block(m, l, Rl, cx.seqs, nc + p.cnt_le[l], p.maxT, a, a.qkv, cache, zf, st, false, Rc,
                        p.single_rows ? nc : INT_MAX));
      TVR_TRY(run_block_out(m, l, Rl, a, st));
    }
  }
  a.resid_mirror = a.qkv_mirror = nullptr;
  a.mirror_rows = 0;
  if (fused) {
    TVR_HIP(hipMemcpyAsync(trace->resid + L * tstride, a.resid, (size_t)Rc * d * sizeof(float),
                           hipMemcpyDeviceToDevice, st));
    trace->pending = false;
  }
  TVR_TRY(sweep_enter(cx, L, trace->resid, trace->z, tstride));
  TVR_TRY(run_final(m, a.resid, (const int32_t*)(base + o_last), (const int32_t*)(base + o_tg), n_sites,
                    (float*)(base + o_xf), (float*)(base + o_lg), out_prob, out_topk, topk, out_logits, fmt, st));
  if (fused && (trace->p_prob || trace->p_topk))
    TVR_TRY(run_final(m, a.resid, (const int32_t*)(base + o_clast), (const int32_t*)(base + o_ctg), nc,
                      (float*)(base + o_xf), (float*)(base + o_lg), trace->p_prob, trace->p_topk, trace->p_k,
                      nullptr, fmt, st));
  return TVR_OK;
}

int tvr_patch_sweep(tvr_model* m, tvr_trace* trace, const tvr_site* sites, int32_t n_sites,
                    const float* vectors, int32_t n_vectors, float* out_prob, int32_t* out_topk,
                    int32_t topk, float* out_logits, void* stream) {
  return sweep_impl("tvr_patch_sweep", m, trace, sites, n_sites, nullptr, nullptr, nullptr, nullptr, vectors, n_vectors, out_prob,
                    out_topk, topk, out_logits, stream);
}

int tvr_patch_sweep_sets(tvr_model* m, tvr_trace* trace, const tvr_site* sites, int32_t n_sites,
                         const int32_t* set_off, const tvr_head_patch* patches, const float* vectors,
                         int32_t n_vectors, float* out_prob, int32_t* out_topk, int32_t topk, float* out_logits,
                         void* stream) {
  if (!m || !trace || !sites || n_sites <= 0 || !set_off)
    return fail(TVR_ERR_INVALID, "tvr_patch_sweep_sets: bad argument");
  if (set_off[0] < 0) return fail(TVR_ERR_INVALID, "tvr_patch_sweep_sets: set_off[0] is negative");
  for (int i = 0; i < n_sites; ++i)
    if (set_off[i + 1] < set_off[i])
      return fail(TVR_ERR_INVALID, "tvr_patch_sweep_sets: set_off decreases at site " + std::to_string(i));
  if (set_off[n_sites] > set_off[0] && !patches)
    return fail(TVR_ERR_INVALID, "tvr_patch_sweep_sets: patches is null but the sets are not empty");
  return sweep_impl("tvr_patch_sweep_sets", m, trace, sites, n_sites, set_off, patches, nullptr, nullptr, vectors,
                    n_vectors, out_prob, out_topk, topk, out_logits, stream);
}

int tvr_patch_sweep_knockout(tvr_model* m, tvr_trace* trace, const tvr_site* sites, int32_t n_sites,
                             const int32_t* set_off, const tvr_head_patch* patches, const int32_t* key_off,
                             const int32_t* keys, const float* vectors, int32_t n_vectors, float* out_prob,
                             int32_t* out_topk, int32_t topk, float* out_logits, void* stream) {
  const std::string fn = "tvr_patch_sweep_knockout: ";
  if (!m || !trace || !sites || n_sites <= 0 || !set_off || !key_off) return fail(TVR_ERR_INVALID, fn + "bad argument");
  if (set_off[0] < 0) return fail(TVR_ERR_INVALID, fn + "set_off[0] is negative");
  if (key_off[0] < 0) return fail(TVR_ERR_INVALID, fn + "key_off[0] is negative");
  for (int i = 0; i < n_sites; ++i) {
    if (set_off[i + 1] < set_off[i]) return fail(TVR_ERR_INVALID, fn + "set_off decreases at site " + std::to_string(i));
    if (key_off[i + 1] < key_off[i]) return fail(TVR_ERR_INVALID, fn + "key_off decreases at site " + std::to_string(i));
  }
  if (set_off[n_sites] > set_off[0] && !patches)
    return fail(TVR_ERR_INVALID, fn + "patches is null but the sets are not empty");
  if (key_off[n_sites] > key_off[0] && !keys)
    return fail(TVR_ERR_INVALID, fn + "keys is null but the key lists are not empty");
  return sweep_impl("tvr_patch_sweep_knockout", m, trace, sites, n_sites, set_off, patches, key_off, keys, vectors,
                    n_vectors, out_prob, out_topk, topk, out_logits, stream);
}

int tvr_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t gemm_mode, int32_t flags, int32_t* out) {
  if (M <= 0 || N <= 0 || K <= 0 || !out || (gemm_mode != TVR_GEMM_X2F16 && gemm_mode != TVR_GEMM_BF16) ||
      (flags & ~(TVR_PLAN_GELU | TVR_PLAN_MODEL_SLICED | TVR_PLAN_EXACT16)))
    return fail(TVR_ERR_INVALID, "tvr_gemm_plan: bad argument");
  const int fmt = gemm_mode == TVR_GEMM_X2F16 ? ACT_X2F16 : ACT_BF16;
  if (K % pp_ktile(fmt) != 0) return fail(TVR_ERR_UNSUPPORTED, "tvr_gemm_plan: K not a k-tile multiple");
  const bool sliced = fmt == ACT_X2F16 && pp_sliced_rule(K, (flags & TVR_PLAN_MODEL_SLICED) ? PP_SLICE_MIN_K : 0);
  const PpPlan p = plan_pp(M, N, K, fmt, (flags & TVR_PLAN_GELU) ? EPI_SPLIT_GELU_ACT : EPI_RESID, sliced,
                           fmt == ACT_X2F16 && (flags & TVR_PLAN_EXACT16));
  out[0] = p.ksplit;
  out[1] = p.tail_base;
  out[2] = p.tail_split;
  out[3] = p.sk_base;
  out[4] = p.sk_blocks;
  return TVR_OK;
}

int tvr_project_heads(tvr_model* m, const float* zsum, float* out, void* stream) {
  if (!m || !zsum || !out) return fail(TVR_ERR_INVALID, "tvr_project_heads: null argument");
  const tvr_config& c = m->cfg;
  hipLaunchKernelGGL(project_heads_kernel, dim3((c.d_model + 255) / 256, c.n_heads, c.n_layers),
                     dim3(256), 0, (hipStream_t)stream, zsum, m->d_w2s, m->K2, out, c.n_heads,
                     c.d_model, c.d_head);
  TVR_HIP(hipGetLastError());
  return TVR_OK;
}

int tvr_gemm_f32(const float* A, int32_t lda, const float* W, int32_t ldw, const float* bias, float* C,
                 int32_t ldc, int32_t M, int32_t N, int32_t K, void* stream) {
  if (!A || !W || !C || M < 0 || N < 0 || K <= 0) return fail(TVR_ERR_INVALID, "tvr_gemm_f32: bad argument");
  GemmEpi e{};
  e.bias = bias;
  e.out0 = C;
  e.ld0 = ldc;
  return launch_gemm(EPI_BIAS, A, lda, ACT_F32, MatW{W}, ldw, M, N, K, e, (hipStream_t)stream);
}

int tvr_split_planes(const float* w, uint16_t* out, size_t n, void* stream) {
  if (!w || !out) return fail(TVR_ERR_INVALID, "tvr_split_planes: null argument");
  if (n == 0) return TVR_OK;
  hipLaunchKernelGGL(split_planes_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, w, out, n);
  TVR_HIP(hipGetLastError());
  return TVR_OK;
}

int tvr_gemm_x3bf16(const float* A, int32_t lda, const uint16_t* W, int32_t ldw, size_t wps,
                    const float* bias, float* C, int32_t ldc, int32_t M, int32_t N, int32_t K, void* stream) {
  if (!A || !W || !C || M < 0 || N < 0 || K <= 0 || wps < (size_t)ldw * (N > 0 ? N - 1 : 0) + K)
    return fail(TVR_ERR_INVALID, "tvr_gemm_x3bf16: bad argument");
  GemmEpi e{};
  e.bias = bias;
  e.out0 = C;
  e.ld0 = ldc;
  return launch_gemm(EPI_BIAS, A, lda, ACT_F32, MatW{nullptr, W, nullptr, wps, 1.0f}, ldw, M, N, K, e,
                     (hipStream_t)stream);
}

int tvr_weight_planes(int32_t fmt, const float* w, float scale, uint16_t* out, size_t n, void* stream) {
  if (!w || !out || (fmt != TVR_GEMM_X2F16 && fmt != TVR_GEMM_BF16))
    return fail(TVR_ERR_INVALID, "tvr_weight_planes: bad argument");
  if (n == 0) return TVR_OK;
  if (fmt == TVR_GEMM_X2F16)
    hipLaunchKernelGGL(split_planes_f16_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, w, scale, out, n);
  else
    hipLaunchKernelGGL(bf16_plane_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, w, out, n, 0);
  TVR_HIP(hipGetLastError());
  return TVR_OK;
}

int tvr_gemm_x2f16(const float* A, int32_t lda, const uint16_t* W, int32_t ldw, size_t wps, float w_scale,
                   const float* bias, float* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                   uint32_t* range_flag, void* stream) {
  if (!A || !W || !C || M < 0 || N < 0 || K <= 0 || !(w_scale > 0.0f) ||
      wps < (size_t)ldw * (N > 0 ? N - 1 : 0) + K)
    return fail(TVR_ERR_INVALID, "tvr_gemm_x2f16: bad argument");
  GemmEpi e{};
  e.bias = bias;
  e.out0 = C;
  e.ld0 = ldc;
  return launch_gemm(EPI_BIAS, A, lda, ACT_F32, MatW{nullptr, nullptr, W, wps, w_scale}, ldw, M, N, K, e,
                     (hipStream_t)stream, nullptr, range_flag);
}

int tvr_act_rows(int32_t fmt, const float* a, int32_t lda, uint16_t* out, int32_t rows, int32_t K,
                 uint32_t* range_flag, void* stream) {
  if (!a || !out || rows < 0 || K <= 0 || lda < K ||
      (fmt != TVR_GEMM_X2F16 && fmt != TVR_GEMM_BF16 && fmt != TVR_ACT_X2F16_IL) ||
      (fmt == TVR_ACT_X2F16_IL && K % 32 != 0))
    return fail(TVR_ERR_INVALID, "tvr_act_rows: bad argument");
  const size_t n = (size_t)rows * K;
  if (n == 0) return TVR_OK;
  const dim3 grid((unsigned)std::min<size_t>((n + 255) / 256, 8192)), block(256);
  if (fmt == TVR_GEMM_X2F16)
    hipLaunchKernelGGL(act_rows_kernel<ACT_X2F16>, grid, block, 0, (hipStream_t)stream, a, lda, out, rows, K, range_flag);
  else if (fmt == TVR_ACT_X2F16_IL)
    hipLaunchKernelGGL(act_rows_kernel<ACT_X2F16I>, grid, block, 0, (hipStream_t)stream, a, lda, out, rows, K, range_flag);
  else
    hipLaunchKernelGGL(act_rows_kernel<ACT_BF16>, grid, block, 0, (hipStream_t)stream, a, lda, out, rows, K, range_flag);
  TVR_HIP(hipGetLastError());
  return TVR_OK;
}

int tvr_gemm_planar(int32_t fmt, const uint16_t* A, int32_t lda, const uint16_t* W, int32_t ldw, size_t wps,
                    float w_scale, const float* bias, float* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                    void* stream) {
  if (!A || !W || !C || M < 0 || N < 0 || K <= 0 || lda < K || !(w_scale > 0.0f) ||
      (fmt != TVR_GEMM_X2F16 && fmt != TVR_GEMM_BF16 && fmt != TVR_ACT_X2F16_IL) ||
      wps < (size_t)ldw * (N > 0 ? N - 1 : 0) + K)
    return fail(TVR_ERR_INVALID, "tvr_gemm_planar: bad argument");
  GemmEpi e{};
  e.bias = bias;
  e.out0 = C;
  e.ld0 = ldc;
  return launch_gemm(EPI_BIAS, A, lda,
                     fmt == TVR_GEMM_X2F16 ? ACT_X2F16 : fmt == TVR_ACT_X2F16_IL ? ACT_X2F16I : ACT_BF16,
                     MatW{nullptr, nullptr, W, wps, w_scale}, ldw, M, N, K, e, (hipStream_t)stream);
}

int tvr_gemm_launch(tvr_model* m, const tvr_gemm_args* a, void* stream) {
  // every check on the host, before any device call and before the model is read
  auto bad = [](const std::string& what) { return fail(TVR_ERR_INVALID, "tvr_gemm_launch: " + what); };
  if (!m) return bad("null model");
  if (!a) return bad("null args");
  if (a->fmt != TVR_GEMM_X2F16 && a->fmt != TVR_ACT_X2F16_IL && a->fmt != TVR_GEMM_BF16)
    return bad("unknown fmt " + std::to_string(a->fmt));
  if (a->exact16 < 0 || a->exact16 > 2) return bad("exact16 must be 0, 1 or 2");
  if (a->exact16 == 2 && a->fmt != TVR_ACT_X2F16_IL)
    return bad("exact16 must be 0 or 1 with this fmt: the row-pair-interleaved weight plane (2) takes the "
               "interleaved activation layout");
  if (a->exact16 == 2 && !pp_wil_available())
    return fail(TVR_ERR_UNSUPPORTED, "tvr_gemm_launch: this build has no interleaved-weight kernel (TVR_PP_WX_WIDE 0)");
  if (a->epi != TVR_EPI_BIAS && a->epi != TVR_EPI_GELU && a->epi != TVR_EPI_RESID)
    return bad("unknown epi " + std::to_string(a->epi));
  if (a->form < TVR_FORM_PLAN || a->form > TVR_FORM_STREAMK) return bad("unknown form " + std::to_string(a->form));
  if (a->slicing < TVR_SLICE_MODEL || a->slicing > TVR_SLICE_OFF)
    return bad("unknown slicing " + std::to_string(a->slicing));
  if (a->skinny != 0 && a->skinny != 1) return bad("skinny must be 0 or 1");
  const bool x2 = a->fmt != TVR_GEMM_BF16, il = a->fmt == TVR_ACT_X2F16_IL, x16 = a->exact16 != 0;
  if (x16 && !x2) return bad("one exact fp16 weight plane takes an x2f16 activation format");
  const int M = a->M, N = a->N, K = a->K, ktile = pp_ktile(x2 ? ACT_X2F16 : ACT_BF16);
  if (M <= 0 || N <= 0 || K <= 0) return bad("M, N and K must be positive");
  if (K % ktile != 0) return bad("K must be a multiple of the k-tile (" + std::to_string(ktile) + ")");
  if (!a->A || !a->W || !a->out0) return bad("null A, W or out0");
  if (!(a->w_scale > 0.0f) || !std::isfinite(a->w_scale)) return bad("w_scale must be positive and finite");
  if (a->lda < K || a->lda % (il ? 32 : 8) != 0)
    return bad("lda must be at least K and a multiple of 8 (32 in the interleaved layout)");
  if (a->ldw < K || a->ldw % 8 != 0) return bad("ldw must be at least K and a multiple of 8");
  const bool two_w = x2 && !x16;
  if (two_w && (a->wps % 8 != 0 || a->wps < (uint64_t)a->ldw * (N - 1) + K))
    return bad("wps must hold N rows of ldw and be a multiple of 8");
  if (a->ld0 < N) return bad("ld0 must be at least N");
  if (((uintptr_t)a->A | (uintptr_t)a->a2 | (uintptr_t)a->W | (uintptr_t)a->out0 | (uintptr_t)a->out0m |
       (uintptr_t)a->out1h | (uintptr_t)a->raw | (uintptr_t)a->resid) & 15)
    return bad("A, a2, W, out0, out0m, out1h, raw and resid must be 16-byte aligned");
  if (((uintptr_t)a->bias | (uintptr_t)a->range_flag) & 3) return bad("bias and range_flag must be 4-byte aligned");
  // rows of the output buffers (out0, out0m, out1h, raw, resid) and of the gather source
  if (a->out_rows && a->out_buf_rows < M) return bad("out_buf_rows must be at least M under out_rows");
  const int orows = a->out_rows ? a->out_buf_rows : M;
  if (a->out_rows) {
    std::vector<char> seen(orows, 0);
    for (int r = 0; r < M; ++r) {
      const int32_t o = a->out_rows[r];
      if (o < 0 || o >= orows) return bad("out_rows[" + std::to_string(r) + "] outside [0, out_buf_rows)");
      if (seen[o]) return bad("out_rows names row " + std::to_string(o) + " twice");
      seen[o] = 1;
    }
  }
  if (a->a_rows) {
    if (a->a_buf_rows <= 0) return bad("a_buf_rows must be positive under a_rows");
    for (int r = 0; r < M; ++r)
      if (a->a_rows[r] < 0 || a->a_rows[r] >= a->a_buf_rows)
        return bad("a_rows[" + std::to_string(r) + "] outside [0, a_buf_rows)");
  }
  if (a->a2 && (a->a2_col < 0 || a->a2_col % 256 != 0)) return bad("a2_col must be a non-negative multiple of 256");
  int mask = N | a->ld0;
  if (a->epi == TVR_EPI_RESID) {
    if (!a->resid) return bad("the residual epilogue needs resid");
    if (a->ldr < N) return bad("ldr must be at least N");
    if (a->out0m) return bad("the residual epilogue has no mirror (out0m)");
    mask |= a->ldr;
  }
  if (a->out0m && (a->mirror_rows < 0 || a->mirror_rows > orows)) return bad("mirror_rows outside [0, output rows]");
  if (a->epi == TVR_EPI_GELU) {
    if (a->n_split < 0 || a->n_split > N) return bad("n_split outside [0, N]");
    const int ng = N - a->n_split;
    if (ng > 0 && !a->out1h) return bad("the GELU epilogue needs out1h");
    if (il ? a->ld1h < 64 * ((ng + 31) / 32)
           : (x2 ? a->ps1h < ng || a->ld1h < a->ps1h + ng : a->ld1h < ng) || a->ps1h < 0)
      return bad("ld1h / ps1h too small for the GELU columns");
    mask |= a->ld1h | a->ps1h | a->n_split;
    // the 8-column GELU stores of a whole tile are 16-byte stores of halves
    if ((mask & 3) == 0 && ((a->ld1h | a->ps1h | a->n_split) & 7) != 0)
      return bad("with the vector epilogue ld1h, ps1h and n_split must be multiples of 8");
    if (a->raw) {
      if (a->out_rows) return bad("raw is addressed by launch row: not with out_rows");
      if (a->raw_rows < 0 || a->raw_rows > M) return bad("raw_rows outside [0, M]");
      if (a->ld_raw < ng || ((mask & 3) == 0 && a->ld_raw % 4 != 0))
        return bad("ld_raw must hold the GELU columns (a multiple of 4 with the vector epilogue)");
    }
  }
  const bool vec = (mask & 3) == 0;
  const bool forced = a->form >= TVR_FORM_SPLITK;
  if (il && !x16 && (a->epi != TVR_EPI_BIAS || forced || a->skinny || a->a2))
    return bad("the interleaved layout with two weight planes runs the plain bias launch only");
  if (a->skinny && (forced || a->out0m || a->epi != TVR_EPI_BIAS))
    return bad("skinny is an opt-in of plain bias launches without a mirror");
  const int tiles = gemm_pingpong_grid(M, N), nkt = K / ktile;
  GemmForce force;
  force.slicing = a->slicing;
  if (a->form != TVR_FORM_PLAN) force.plan_set = true;  // TVR_FORM_PLAIN: the default PpPlan
  if (forced) {
    if (!vec) return bad("a split or stream-K launch needs the vector epilogue (N and the strides multiples of 4)");
    if (a->form == TVR_FORM_STREAMK) {
      if (a->form_tile < 0 || a->form_tile >= tiles) return bad("form_tile outside the raster");
      const int cnt = tiles - a->form_tile;
      if (a->form_n < cnt || a->form_n > 256 || (long long)a->form_n > (long long)cnt * nkt)
        return bad("stream-K blocks outside [tiles, min(256, tiles x k-tiles)]");
      force.plan.sk_base = a->form_tile;
      force.plan.sk_blocks = a->form_n;
    } else {
      const bool tail = a->form == TVR_FORM_TAIL;
      if (tail && (a->form_tile < 1 || a->form_tile >= tiles)) return bad("form_tile outside the raster");
      const int cnt = tail ? tiles - a->form_tile : tiles, S = a->form_n;
      if (S < 2 || nkt / S < 8) return bad("split S must be at least 2 with at least 8 k-tiles per part");
      if ((long long)cnt * S > 4096) return bad("more partial tiles than the workspace cap (4096)");
      if (tail) {
        force.plan.tail_base = a->form_tile;
        force.plan.tail_split = S;
      } else {
        force.plan.ksplit = S;
      }
    }
  }
  const hipStream_t st = (hipStream_t)stream;
  GemmEpi e{};
  e.bias = a->bias;
  e.out0 = a->out0;
  e.ld0 = a->ld0;
  e.n_split = a->n_split;
  e.resid = a->resid;
  e.ldr = a->ldr;
  e.out1h = a->out1h;
  e.ld1h = a->ld1h;
  e.ps1h = a->ps1h;
  e.range_flag = a->range_flag;
  if (a->epi == TVR_EPI_GELU) {
    e.raw = a->raw;
    e.raw_rows = a->raw_rows;
    e.ld_raw = a->ld_raw;
  }
  e.out0m = a->out0m;
  e.mirror_rows = a->mirror_rows;
  e.a2 = a->a2;
  e.a2_col = a->a2_col;
  e.skinny = a->skinny;
  // the row indices are host arrays (checked above): one temporary device buffer for both
  int32_t* d_rows = nullptr;
  int rc = TVR_OK;
  if (a->a_rows || a->out_rows) {
    if (hipMalloc(&d_rows, (size_t)2 * M * sizeof(int32_t)) != hipSuccess)
      return fail(TVR_ERR_NOMEM, "tvr_gemm_launch: row index buffer");
    hipError_t err = hipSuccess;
    if (a->a_rows) err = hipMemcpyAsync(d_rows, a->a_rows, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (err == hipSuccess && a->out_rows)
      err = hipMemcpyAsync(d_rows + M, a->out_rows, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);  // pageable host memory
    if (err != hipSuccess) rc = fail(TVR_ERR_HIP, std::string("tvr_gemm_launch: ") + hipGetErrorString(err));
    if (a->a_rows) e.a_rows = d_rows;
    if (a->out_rows) e.out_rows = d_rows + M;
  }
  if (rc == TVR_OK) {
    const int epi = a->epi == TVR_EPI_BIAS ? EPI_BIAS : a->epi == TVR_EPI_GELU ? EPI_SPLIT_GELU_ACT : EPI_RESID;
    const int afmt = il ? ACT_X2F16I : x2 ? ACT_X2F16 : ACT_BF16;
    // (exact16 2: the caller's plane is the interleaved one; launch_gemm's form for it is checked above)
    MatW W{nullptr, nullptr, a->W, (size_t)a->wps, x2 ? a->w_scale : 1.0f, x16, a->exact16 == 2 ? a->W : nullptr};
    // (two weight planes in the interleaved layout: launch_gemm takes them without a model only)
    rc = launch_gemm(epi, a->A, a->lda, afmt, W, a->ldw, M, N, K, e, st, il && !x16 ? nullptr : m, nullptr, &force);
    if (rc == TVR_OK) {
      const hipError_t err = hipGetLastError();
      if (err != hipSuccess) rc = fail(TVR_ERR_HIP, std::string("tvr_gemm_launch: ") + hipGetErrorString(err));
    }
  }
  const hipError_t err = hipStreamSynchronize(st);
  if (rc == TVR_OK && err != hipSuccess) rc = fail(TVR_ERR_HIP, std::string("tvr_gemm_launch: ") + hipGetErrorString(err));
  if (d_rows) (void)hipFree(d_rows);
  return rc;
}

int tvr_lnpre_f32(const float* x, int32_t ldx, float* y, int32_t ldy, int32_t rows, int32_t d, float eps,
                  void* stream) {
  if (!x || !y || rows < 0 || d <= 0) return fail(TVR_ERR_INVALID, "tvr_lnpre_f32: bad argument");
  return launch_lnpre(x, ldx, nullptr, y, ldy, rows, d, eps, ACT_F32, (hipStream_t)stream);
}

int tvr_lnpre_rows(tvr_model* m, const tvr_lnpre_args* a, void* stream) {
  // every check on the host, before any device call: a wrong argument never becomes a device access
  auto bad = [](const std::string& what) { return fail(TVR_ERR_INVALID, "tvr_lnpre_rows: " + what); };
  if (!a) return bad("null args");
  if (!a->x) return bad("null x");
  if (!a->y) return bad("null y");
  const int fmt = a->fmt, rows = a->rows, d = a->d;
  if (fmt != 0 && fmt != TVR_GEMM_X2F16 && fmt != TVR_ACT_X2F16_IL && fmt != TVR_GEMM_BF16)
    return bad("unknown fmt " + std::to_string(fmt));
  if (rows <= 0) return bad("rows must be positive");
  if (d <= 0 || d % 4 != 0 || a->ldx % 4 != 0 || a->ldy % 4 != 0) return bad("d, ldx and ldy must be positive multiples of 4");
  if (a->ldx < d || a->ldy < d) return bad("ldx and ldy must be at least d");
  if (fmt == TVR_ACT_X2F16_IL && (d % 32 != 0 || a->ldy % 32 != 0))
    return bad("the interleaved format needs d and ldy to be multiples of 32");
  if (((uintptr_t)a->x | (uintptr_t)a->y | (uintptr_t)a->y2 | (uintptr_t)a->copy | (uintptr_t)a->g1 | (uintptr_t)a->g2) & 15)
    return bad("x, y, y2, copy and the gammas must be 16-byte aligned");
  if ((uintptr_t)a->stats & 7) return bad("stats must be 8-byte aligned");
  if (a->x_rows <= 0) return bad("x_rows must be positive");
  if (a->row_idx) {
    for (int r = 0; r < rows; ++r)
      if (a->row_idx[r] < 0 || a->row_idx[r] >= a->x_rows)
        return bad("row_idx[" + std::to_string(r) + "] outside [0, x_rows)");
  } else if (rows > a->x_rows) {
    return bad("rows exceeds x_rows without row_idx");
  }
  if (a->copy_rows < 0) return bad("copy_rows is negative");
  if (a->copy_rows > 0 && !a->copy) return bad("copy_rows given with a null copy");
  const bool x2 = fmt == TVR_GEMM_X2F16 || fmt == TVR_ACT_X2F16_IL;
  if (a->g1 && !x2) return bad("the gamma-scaled rows are x2f16 formats only");
  if (a->g1 && !m) return bad("g1 needs a model (its range flag)");
  if (a->y2 && (!a->g1 || !a->g2)) return bad("y2 needs g1 and g2");
  if (a->g2 && !a->y2) return bad("g2 needs y2");

  const int afmt = fmt == 0 ? ACT_F32 : fmt == TVR_GEMM_X2F16 ? ACT_X2F16 : fmt == TVR_ACT_X2F16_IL ? ACT_X2F16I : ACT_BF16;
  const hipStream_t st = (hipStream_t)stream;
  int32_t* d_idx = nullptr;
  int rc = TVR_OK;
  if (a->row_idx) {
    if (hipMalloc(&d_idx, (size_t)rows * sizeof(int32_t)) != hipSuccess)
      return fail(TVR_ERR_NOMEM, "tvr_lnpre_rows: row index buffer");
    hipError_t e = hipMemcpyAsync(d_idx, a->row_idx, (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // row_idx is pageable host memory
    if (e != hipSuccess) rc = fail(TVR_ERR_HIP, std::string("tvr_lnpre_rows: ") + hipGetErrorString(e));
  }
  if (rc == TVR_OK)
    rc = launch_lnpre(a->x, a->ldx, d_idx, a->y, a->ldy, rows, d, a->eps, afmt, st, m, reinterpret_cast<float2*>(a->stats),
                      a->copy, a->copy_rows, a->g1, a->g2, a->y2);
  const hipError_t e = hipStreamSynchronize(st);
  if (rc == TVR_OK && e != hipSuccess) rc = fail(TVR_ERR_HIP, std::string("tvr_lnpre_rows: ") + hipGetErrorString(e));
  if (d_idx) (void)hipFree(d_idx);
  return rc;
}

int tvr_center_rows(const float* src, float* dst, int32_t rows, int32_t d, void* stream) {
  auto bad = [](const std::string& what) { return fail(TVR_ERR_INVALID, "tvr_center_rows: " + what); };
  if (!src || !dst) return bad("null src or dst");
  if (rows <= 0 || d <= 0) return bad("rows and d must be positive");
  if (((uintptr_t)src | (uintptr_t)dst) & 3) return bad("src and dst must be float aligned");
  const size_t n = (size_t)rows * d;
  if (src != dst && src < dst + n && dst < src + n) return bad("src and dst overlap without being equal");
  TVR_TRY(launch_center_rows(src, dst, rows, d, (hipStream_t)stream));
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail(TVR_ERR_HIP, "tvr_center_rows: the launch failed");
  return TVR_OK;
}

static_assert(sizeof(tvr_attn_seq) == sizeof(SeqDesc), "tvr_attn_seq is SeqDesc");

int tvr_attention(tvr_model* m, int32_t fmt, const float* qkv, const float* cache, const tvr_attn_seq* seqs,
                  int32_t n_seq, int32_t row_from, int32_t rows, int32_t cache_rows, void* z, float* zf,
                  int32_t zf_last, int32_t zf_rows, const float* cos_t, const float* sin_t, void* stream) {
  // every check on the host, before any device call: a wrong descriptor never becomes a device read
  auto bad = [](const std::string& what) { return fail(TVR_ERR_INVALID, "tvr_attention: " + what); };
  if (!m) return bad("null model");
  if (!qkv) return bad("null qkv");
  if (!z) return bad("null z");
  if (!seqs) return bad("null seqs");
  if (n_seq <= 0) return bad("n_seq must be positive");
  if (fmt != 0 && fmt != TVR_GEMM_X2F16 && fmt != TVR_ACT_X2F16_IL && fmt != TVR_GEMM_BF16)
    return bad("unknown fmt " + std::to_string(fmt));
  if (fmt == TVR_ACT_X2F16_IL && m->K2 % 32 != 0) return bad("the interleaved format needs K2 % 32 == 0");
  if (rows <= 0 || cache_rows < 0) return bad("rows must be positive and cache_rows non-negative");
  if (zf_rows < 0) return bad("zf_rows is negative");  // the kernels compare it as size_t
  if (row_from < 0 || row_from > n_seq) return bad("row_from outside [0, n_seq]");
  if ((cos_t == nullptr) != (sin_t == nullptr)) return bad("cos_t and sin_t must both be given or both be null");
  if (((uintptr_t)qkv | (uintptr_t)cache | (uintptr_t)z | (uintptr_t)zf) & 15)
    return bad("qkv, cache, z and zf must be 16-byte aligned");
  const int n_ctx = m->cfg.n_ctx;
  int maxT = 0;
  for (int s = 0; s < n_seq; ++s) {
    const tvr_attn_seq& q = seqs[s];
    const std::string at = " (sequence " + std::to_string(s) + ")";
    if (q.n < 1) return bad("n must be at least 1" + at);
    if (q.q0 < 0 || q.q0 >= q.n) return bad("q0 outside [0, n)" + at);
    if (q.p0 < 0) return bad("p0 is negative" + at);
    if ((int64_t)q.p0 + q.n > n_ctx) return bad("p0 + n exceeds n_ctx" + at);
    if (q.row0 < 0 || (int64_t)q.row0 + q.n > rows) return bad("rows [row0, row0 + n) outside the qkv buffer" + at);
    if (q.prefix_live != 0 && q.prefix_live != 1) return bad("prefix_live must be 0 or 1" + at);
    if (q.p0 > 0) {
      if (q.cache_row < 0) return bad("cache_row is negative with p0 > 0" + at);
      if (q.prefix_live == 0 && !cache) return bad("null cache with p0 > 0 and prefix_live 0" + at);
      if ((int64_t)q.cache_row + q.p0 > (q.prefix_live ? rows : cache_rows))
        return bad(std::string("prefix rows [cache_row, cache_row + p0) outside the ") +
                   (q.prefix_live ? "qkv" : "cache") + " buffer" + at);
    }
    if (s >= row_from && q.q0 != q.n - 1) return bad("a sequence at or after row_from needs q0 == n - 1" + at);
    maxT = std::max(maxT, q.p0 + q.n);
  }
  const int afmt = fmt == 0 ? ACT_F32 : fmt == TVR_GEMM_X2F16 ? ACT_X2F16 : fmt == TVR_ACT_X2F16_IL ? ACT_X2F16I : ACT_BF16;
  const hipStream_t st = (hipStream_t)stream;
  SeqDesc* d_seqs = nullptr;
  if (hipMalloc(&d_seqs, (size_t)n_seq * sizeof(SeqDesc)) != hipSuccess)
    return fail(TVR_ERR_NOMEM, "tvr_attention: descriptor buffer");
  hipError_t e = hipMemcpyAsync(d_seqs, seqs, (size_t)n_seq * sizeof(SeqDesc), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // seqs is pageable host memory
  int rc = e == hipSuccess ? TVR_OK : fail(TVR_ERR_HIP, std::string("tvr_attention: ") + hipGetErrorString(e));
  if (rc == TVR_OK)
    rc = launch_attention(m, qkv, cache, d_seqs, n_seq, maxT, z, afmt, zf, st, zf_last != 0, zf_rows, row_from, cos_t,
                          sin_t);
  e = hipStreamSynchronize(st);
  if (rc == TVR_OK && e != hipSuccess) rc = fail(TVR_ERR_HIP, std::string("tvr_attention: ") + hipGetErrorString(e));
  (void)hipFree(d_seqs);
  return rc;
}

int tvr_attention_knockout(tvr_model* m, int32_t fmt, const float* qkv, const float* cache, const tvr_attn_seq* seqs,
                           int32_t n_seq, int32_t rows, int32_t cache_rows, const tvr_knockout_item* items,
                           int32_t n_items, const int32_t* keys, int32_t n_keys, void* z, const float* cos_t,
                           const float* sin_t, void* stream) {
  // every check on the host, before any device call
  const char* fn = "tvr_attention_knockout";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!m) return bad("null model");
  if (!qkv) return bad("null qkv");
  if (!z) return bad("null z");
  if (!seqs) return bad("null seqs");
  if (!items) return bad("null items");
  if (n_seq <= 0) return bad("n_seq must be positive");
  if (n_items <= 0) return bad("n_items must be positive");
  if (n_keys < 0 || (n_keys > 0 && !keys)) return bad("n_keys is negative, or keys is null");
  if (fmt != 0 && fmt != TVR_GEMM_X2F16 && fmt != TVR_ACT_X2F16_IL && fmt != TVR_GEMM_BF16)
    return bad("unknown fmt " + std::to_string(fmt));
  if (fmt == TVR_ACT_X2F16_IL && m->K2 % 32 != 0) return bad("the interleaved format needs K2 % 32 == 0");
  if (rows <= 0 || cache_rows < 0) return bad("rows must be positive and cache_rows non-negative");
  if ((cos_t == nullptr) != (sin_t == nullptr)) return bad("cos_t and sin_t must both be given or both be null");
  if (((uintptr_t)qkv | (uintptr_t)cache | (uintptr_t)z | (uintptr_t)cos_t | (uintptr_t)sin_t) & 15)
    return bad("qkv, cache, z and the rotary tables must be 16-byte aligned");
  const tvr_config& c = m->cfg;
  for (int s = 0; s < n_seq; ++s) {
    const tvr_attn_seq& q = seqs[s];
    const std::string at = " (sequence " + std::to_string(s) + ")";
    if (q.n < 1) return bad("n must be at least 1" + at);
    if (q.p0 < 0) return bad("p0 is negative" + at);
    if ((int64_t)q.p0 + q.n > c.n_ctx) return bad("p0 + n exceeds n_ctx" + at);
    if (q.row0 < 0 || (int64_t)q.row0 + q.n > rows) return bad("rows [row0, row0 + n) outside the qkv buffer" + at);
    if (q.prefix_live != 0 && q.prefix_live != 1) return bad("prefix_live must be 0 or 1" + at);
    if (q.p0 > 0) {
      if (q.cache_row < 0) return bad("cache_row is negative with p0 > 0" + at);
      if (q.prefix_live == 0 && !cache) return bad("null cache with p0 > 0 and prefix_live 0" + at);
      if ((int64_t)q.cache_row + q.p0 > (q.prefix_live ? rows : cache_rows))
        return bad(std::string("prefix rows [cache_row, cache_row + p0) outside the ") +
                   (q.prefix_live ? "qkv" : "cache") + " buffer" + at);
    }
  }
  if (c.n_heads > 64) return fail(TVR_ERR_UNSUPPORTED, std::string(fn) + ": the knockout head mask covers 64 heads");
  std::vector<KnockoutItem> kitems(n_items);
  std::vector<uint32_t> masks;
  std::map<int, uint64_t> listed;  // z row -> heads some item writes
  int max_keys = 0;
  for (int i = 0; i < n_items; ++i) {
    const tvr_knockout_item& it = items[i];
    const std::string at = " (item " + std::to_string(i) + ")";
    if (it.seq < 0 || it.seq >= n_seq) return bad("seq out of range" + at);
    if (c.n_heads < 64 && (it.heads >> c.n_heads) != 0) return bad("head mask names a head outside [0, n_heads)" + at);
    if (it.first_key < 0 || it.n_keys < 0 || (int64_t)it.first_key + it.n_keys > n_keys)
      return bad("key range outside the list" + at);
    const int T = seqs[it.seq].p0 + seqs[it.seq].n, zrow = seqs[it.seq].row0 + seqs[it.seq].n - 1;
    if (it.n_keys >= T) return bad("every key is blocked: one key of the last query must remain" + at);
    const int mask_off = (int)masks.size();
    masks.resize(mask_off + (T + 31) / 32, 0u);
    for (int q = it.first_key; q < it.first_key + it.n_keys; ++q) {
      if (keys[q] < 0 || keys[q] >= T) return bad("blocked key outside [0, p0 + n)" + at);
      if (q > it.first_key && keys[q] <= keys[q - 1]) return bad("blocked keys must be strictly increasing" + at);
      masks[mask_off + keys[q] / 32] |= 1u << (keys[q] % 32);
    }
    uint64_t& seen = listed[zrow];
    if (seen & it.heads) return bad("two items list the same head of one row" + at);
    seen |= it.heads;
    kitems[i] = KnockoutItem{it.seq, mask_off, (uint32_t)it.heads, (uint32_t)(it.heads >> 32)};
    max_keys = std::max(max_keys, T);
  }
  TVR_TRY(check_knockout(c, fn, max_keys));

  const hipStream_t st = (hipStream_t)stream;
  const size_t b_seqs = align_up((size_t)n_seq * sizeof(SeqDesc)), b_items = align_up((size_t)n_items * sizeof(KnockoutItem));
  char* dbuf = nullptr;
  if (hipMalloc(&dbuf, b_seqs + b_items + masks.size() * sizeof(uint32_t) + kAlign) != hipSuccess) {
    (void)hipGetLastError();
    return fail(TVR_ERR_NOMEM, std::string(fn) + ": descriptor buffer");
  }
  hipError_t e = hipMemcpyAsync(dbuf, seqs, (size_t)n_seq * sizeof(SeqDesc), hipMemcpyHostToDevice, st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(dbuf + b_seqs, kitems.data(), (size_t)n_items * sizeof(KnockoutItem), hipMemcpyHostToDevice, st);
  if (e == hipSuccess)
    e = hipMemcpyAsync(dbuf + b_seqs + b_items, masks.data(), masks.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // pageable host memory
  int rc = e == hipSuccess ? TVR_OK : fail(TVR_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  Acts a{nullptr, nullptr, const_cast<float*>(qkv), (float*)z,
         fmt == 0 ? ACT_F32 : fmt == TVR_GEMM_X2F16 ? ACT_X2F16 : fmt == TVR_ACT_X2F16_IL ? ACT_X2F16I : ACT_BF16};
  a.ko_seqs = (const SeqDesc*)dbuf;
  a.ko_items = (const KnockoutItem*)(dbuf + b_seqs);
  a.ko_masks = (const uint32_t*)(dbuf + b_seqs + b_items);
  a.ko_cache = cache;
  a.ko_n = n_items;
  a.ko_max_keys = max_keys;
  if (rc == TVR_OK) rc = apply_knockout(m, a, st, cos_t, sin_t);
  e = hipStreamSynchronize(st);
  if (rc == TVR_OK && e != hipSuccess) rc = fail(TVR_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  (void)hipFree(dbuf);
  return rc;
}

int tvr_attention_pattern(tvr_model* m, const float* qkv, int32_t rows, const int32_t* row0, const int32_t* qpos,
                          int32_t n_seq, const int32_t* cls, int32_t n_classes, float* out_pattern, int32_t ld,
                          float* out_mass, const float* cos_t, const float* sin_t, void* stream) {
  // every check on the host, before any device call
  const char* fn = "tvr_attention_pattern";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!m) return bad("null model");
  if (!qkv) return bad("null qkv");
  if (!row0 || !qpos) return bad("null row0 / qpos");
  if (n_seq <= 0) return bad("n_seq must be positive");
  if (rows <= 0) return bad("rows must be positive");
  TVR_TRY(check_pattern_args(fn, cls, rows, n_classes, out_pattern, out_mass));
  if ((cos_t == nullptr) != (sin_t == nullptr)) return bad("cos_t and sin_t must both be given or both be null");
  if (((uintptr_t)qkv | (uintptr_t)cos_t | (uintptr_t)sin_t) & 15)
    return bad("qkv and the rotary tables must be 16-byte aligned");
  std::vector<PatternSeq> seqs(n_seq);
  int max_q = 0;
  for (int s = 0; s < n_seq; ++s) {
    const std::string at = " (sequence " + std::to_string(s) + ")";
    if (qpos[s] < 0 || qpos[s] >= m->cfg.n_ctx) return bad("qpos outside [0, n_ctx)" + at);
    if (row0[s] < 0 || (int64_t)row0[s] + qpos[s] >= rows) return bad("rows [row0, row0 + qpos] outside the qkv buffer" + at);
    seqs[s] = PatternSeq{row0[s], qpos[s]};
    max_q = std::max(max_q, qpos[s]);
  }
  if (out_pattern && ld <= max_q) return bad("ld must exceed the largest query position (" + std::to_string(max_q) + ")");
  const hipStream_t st = (hipStream_t)stream;
  // descriptors, then the classes, in one temporary buffer
  const size_t seq_bytes = align_up((size_t)n_seq * sizeof(PatternSeq));
  const size_t cls_bytes = out_mass ? (size_t)rows * sizeof(int32_t) : 0;
  char* dbuf = nullptr;
  if (hipMalloc(&dbuf, seq_bytes + cls_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(TVR_ERR_NOMEM, std::string(fn) + ": descriptor buffer");
  }
  hipError_t e = hipMemcpyAsync(dbuf, seqs.data(), (size_t)n_seq * sizeof(PatternSeq), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && cls_bytes) e = hipMemcpyAsync(dbuf + seq_bytes, cls, cls_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // pageable host memory
  int rc = e == hipSuccess ? TVR_OK : fail(TVR_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  if (rc == TVR_OK)
    rc = launch_pattern(m, fn, qkv, 0, 1, (const PatternSeq*)dbuf, n_seq, max_q + 1,
                        cls_bytes ? (const int32_t*)(dbuf + seq_bytes) : nullptr, n_classes, out_pattern, ld, out_mass,
                        cos_t, sin_t, st);
  e = hipStreamSynchronize(st);
  if (rc == TVR_OK && e != hipSuccess) rc = fail(TVR_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  (void)hipFree(dbuf);
  return rc;
}

int tvr_attention_source(tvr_model* m, const float* qkv, int32_t rows, const int32_t* row0, const int32_t* qpos,
                         int32_t n_seq, const float* g, const int32_t* cls, int32_t n_classes, float* out_src,
                         int32_t ld, float* out_cls, const float* cos_t, const float* sin_t, void* stream) {
  // every check on the host, before any device call
  const char* fn = "tvr_attention_source";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!m) return bad("null model");
  if (!qkv) return bad("null qkv");
  if (!row0 || !qpos) return bad("null row0 / qpos");
  if (!g) return bad("null g");
  if (n_seq <= 0) return bad("n_seq must be positive");
  if (rows <= 0) return bad("rows must be positive");
  TVR_TRY(check_source_args(fn, cls, rows, n_classes, out_src, out_cls));
  if ((cos_t == nullptr) != (sin_t == nullptr)) return bad("cos_t and sin_t must both be given or both be null");
  if (((uintptr_t)qkv | (uintptr_t)g | (uintptr_t)cos_t | (uintptr_t)sin_t) & 15)
    return bad("qkv, g and the rotary tables must be 16-byte aligned");
  std::vector<PatternSeq> seqs(n_seq);
  int max_q = 0;
  for (int s = 0; s < n_seq; ++s) {
    const std::string at = " (sequence " + std::to_string(s) + ")";
    if (qpos[s] < 0 || qpos[s] >= m->cfg.n_ctx) return bad("qpos outside [0, n_ctx)" + at);
    if (row0[s] < 0 || (int64_t)row0[s] + qpos[s] >= rows) return bad("rows [row0, row0 + qpos] outside the qkv buffer" + at);
    seqs[s] = PatternSeq{row0[s], qpos[s]};
    max_q = std::max(max_q, qpos[s]);
  }
  if (out_src && ld <= max_q) return bad("ld must exceed the largest query position (" + std::to_string(max_q) + ")");
  TVR_TRY(check_source(m->cfg, fn, n_seq, 1, max_q + 1));
  const hipStream_t st = (hipStream_t)stream;
  // descriptors, then the classes, in one temporary buffer
  const size_t seq_bytes = align_up((size_t)n_seq * sizeof(PatternSeq));
  const size_t cls_bytes = out_cls ? (size_t)rows * sizeof(int32_t) : 0;
  char* dbuf = nullptr;
  if (hipMalloc(&dbuf, seq_bytes + cls_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(TVR_ERR_NOMEM, std::string(fn) + ": descriptor buffer");
  }
  hipError_t e = hipMemcpyAsync(dbuf, seqs.data(), (size_t)n_seq * sizeof(PatternSeq), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && cls_bytes) e = hipMemcpyAsync(dbuf + seq_bytes, cls, cls_bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // pageable host memory
  int rc = e == hipSuccess ? TVR_OK : fail(TVR_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  if (rc == TVR_OK)
    rc = launch_source(m, fn, qkv, 0, 1, (const PatternSeq*)dbuf, n_seq, max_q + 1, g, 0,
                       cls_bytes ? (const int32_t*)(dbuf + seq_bytes) : nullptr, n_classes, out_src, ld, out_cls, 0, 1,
                       cos_t, sin_t, st);
  e = hipStreamSynchronize(st);
  if (rc == TVR_OK && e != hipSuccess) rc = fail(TVR_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  (void)hipFree(dbuf);
  return rc;
}

int tvr_site_entry(tvr_model* m, const int32_t* seq_lens, int32_t n_seq, const int32_t* token_ids, int32_t tokens,
                   const float* resid, const float* z, const tvr_site* sites, int32_t n_sites,
                   const int32_t* set_off, const tvr_head_patch* patches, const float* vectors,
                   int32_t n_vectors, int32_t flags, float* out, int32_t out_rows, int32_t* site_row0,
                   int32_t* site_rows, int32_t* site_p0, void* stream) {
  // every check on the host, before any device call
  const char* fn = "tvr_site_entry";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!m) return bad("null model");
  if (!seq_lens) return bad("null seq_lens");
  if (!resid || !z) return bad("null resid / z");
  if (!sites) return bad("null sites");
  if (!out) return bad("null out");
  if (!site_row0 || !site_rows || !site_p0) return bad("null site_row0 / site_rows / site_p0");
  if (n_seq <= 0) return bad("n_seq must be positive");
  if (n_sites <= 0) return bad("n_sites must be positive");
  if (tokens <= 0 || out_rows <= 0) return bad("tokens and out_rows must be positive");
  if (n_vectors < 0) return bad("n_vectors is negative");
  if (flags & ~TVR_ENTRY_FORCE_VALU) return bad("unknown flags " + std::to_string(flags));
  if (((uintptr_t)resid | (uintptr_t)z | (uintptr_t)out) & 15) return bad("resid, z and out must be 16-byte aligned");
  if ((uintptr_t)vectors & 3) return bad("vectors must be float aligned");
  if ((set_off == nullptr) != (patches == nullptr) && !(set_off && set_off[n_sites] <= set_off[0]))
    return bad("set_off and patches must both be given or both be null");
  const tvr_config& c = m->cfg;
  const int d = c.d_model, L = c.n_layers;
  std::vector<int> seq_off(n_seq), seq_len(n_seq);
  int64_t total = 0;
  for (int s = 0; s < n_seq; ++s) {
    if (seq_lens[s] < 1 || seq_lens[s] > c.n_ctx)
      return bad("a length outside [1, n_ctx] (sequence " + std::to_string(s) + ")");
    seq_off[s] = (int)total;
    seq_len[s] = seq_lens[s];
    total += seq_lens[s];
    if (total > tokens) return bad("the layout exceeds tokens (sequence " + std::to_string(s) + ")");
  }
  if (set_off) {
    if (set_off[0] < 0) return bad("set_off[0] is negative");
    for (int i = 0; i < n_sites; ++i)
      if (set_off[i + 1] < set_off[i]) return bad("set_off decreases at site " + std::to_string(i));
  }
  const bool aligned16 = ((uintptr_t)vectors & 15) == 0;
  for (int i = 0; i < n_sites; ++i)
    if (sites[i].kind == TVR_SITE_REPLACE_HEAD_ALLPOS && !aligned16)  // (the plain sweep's planning does not check)
      return bad("site " + std::to_string(i) + ": REPLACE_HEAD_ALLPOS needs 16-byte aligned vectors");
  const SweepPlanIn in{L, c.n_heads, d, c.d_head, seq_off.data(), seq_len.data(), token_ids, n_seq, (int)total,
                       false, token_ids != nullptr && prefix_share_enabled(), false, ENTRY_GROUP, n_vectors,
                       vectors != nullptr, aligned16, 4.0, sites, n_sites, set_off, patches};
  SweepPlan p;
  std::string err;
  if (plan_sweep(in, p, err) != TVR_OK) return bad(err);
  if (p.R > out_rows) return bad("the sites materialise " + std::to_string(p.R) + " rows: more than out_rows");
  for (int i = 0; i < n_sites; ++i) {
    site_row0[i] = p.row0[i];
    site_rows[i] = p.nrow[i];
    site_p0[i] = p.p0[i];
  }

  // the tables the entry kernels read, in one temporary buffer
  const hipStream_t st = (hipStream_t)stream;
  const size_t b_ents = align_up(p.ents.size() * sizeof(EntryDesc)), b_gidx = align_up(p.egidx.size() * sizeof(int32_t));
  const size_t b_groups = p.egroups.size() * sizeof(EntryGroup);
  char* dbuf = nullptr;
  if (hipMalloc(&dbuf, b_ents + b_gidx + b_groups + kAlign) != hipSuccess) {
    (void)hipGetLastError();
    return fail(TVR_ERR_NOMEM, std::string(fn) + ": descriptor buffer");
  }
  hipError_t e = hipMemcpyAsync(dbuf, p.ents.data(), p.ents.size() * sizeof(EntryDesc), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && !p.egidx.empty())
    e = hipMemcpyAsync(dbuf + b_ents, p.egidx.data(), p.egidx.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && b_groups)
    e = hipMemcpyAsync(dbuf + b_ents + b_gidx, p.egroups.data(), b_groups, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // pageable host memory
  int rc = e == hipSuccess ? TVR_OK : fail(TVR_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  // the sites' rows are the activation rows [0, R) (no fused clean rows): the entry kernels write them to `out`
  Acts a{out, nullptr, nullptr, nullptr, ACT_F32};
  const SweepCtx cx{m, nullptr, p, false, a, vectors, st, nullptr, (const EntryDesc*)dbuf,
                    (const int32_t*)(dbuf + b_ents), (const EntryGroup*)(dbuf + b_ents + b_gidx),
                    nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int l = 0; l <= L && rc == TVR_OK; ++l)
    rc = sweep_enter(cx, l, resid, z, (size_t)tokens * d, (flags & TVR_ENTRY_FORCE_VALU) != 0);
  e = hipStreamSynchronize(st);
  if (rc == TVR_OK && e != hipSuccess) rc = fail(TVR_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  (void)hipFree(dbuf);
  return rc;
}

static_assert(sizeof(tvr_headset_item) == sizeof(HeadsetItem) && sizeof(tvr_headset_patch) == sizeof(HeadsetPatch),
              "tvr_headset_item / tvr_headset_patch are HeadsetItem / HeadsetPatch");

int tvr_headset_apply(tvr_model* m, int32_t fmt, const tvr_headset_item* items, int32_t n_items,
                      const tvr_headset_patch* patches, int32_t n_patches, const float* vectors, int32_t n_vectors,
                      void* a2, float* resid, int32_t rows, void* stream) {
  // every check on the host, before any device call
  const char* fn = "tvr_headset_apply";
  auto bad = [&](const std::string& what) { return fail(TVR_ERR_INVALID, std::string(fn) + ": " + what); };
  if (!m) return bad("null model");
  if (!items) return bad("null items");
  if (!vectors) return bad("null vectors");
  if (!a2 || !resid) return bad("null a2 / resid");
  if (n_items <= 0) return bad("n_items must be positive");
  if (n_patches < 0 || (n_patches > 0 && !patches)) return bad("n_patches is negative, or patches is null");
  if (rows <= 0) return bad("rows must be positive");
  if (n_vectors < 0) return bad("n_vectors is negative");
  if (fmt != 0 && fmt != TVR_GEMM_X2F16 && fmt != TVR_ACT_X2F16_IL && fmt != TVR_GEMM_BF16)
    return bad("unknown fmt " + std::to_string(fmt));
  if (fmt == TVR_ACT_X2F16_IL && m->K2 % 32 != 0) return bad("the interleaved format needs K2 % 32 == 0");
  if (((uintptr_t)a2 | (uintptr_t)resid) & 15) return bad("a2 and resid must be 16-byte aligned");
  if ((uintptr_t)vectors & 3) return bad("vectors must be float aligned");
  const tvr_config& c = m->cfg;
  std::vector<std::pair<int64_t, int64_t>> spans;
  int max_rows = 0;
  for (int i = 0; i < n_items; ++i) {
    const tvr_headset_item& it = items[i];
    const std::string at = " (item " + std::to_string(i) + ")";
    if (it.n_rows < 1) return bad("n_rows must be at least 1" + at);
    if (it.row0 < 0 || (int64_t)it.row0 + it.n_rows > rows) return bad("rows [row0, row0 + n_rows) outside the buffers" + at);
    if (it.first_patch < 0 || it.n_patches < 0 || (int64_t)it.first_patch + it.n_patches > n_patches)
      return bad("patch range outside the list" + at);
    for (int q = it.first_patch; q < it.first_patch + it.n_patches; ++q) {
      if (patches[q].head < 0 || patches[q].head >= c.n_heads) return bad("head out of range" + at);
      if (patches[q].vec < 0 || patches[q].vec >= n_vectors) return bad("vector out of range" + at);
    }
    spans.emplace_back(it.row0, (int64_t)it.row0 + it.n_rows);
    max_rows = std::max(max_rows, it.n_rows);
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].first < spans[i - 1].second) return bad("two items share rows");  // (their residual sums would race)

  const hipStream_t st = (hipStream_t)stream;
  const size_t b_items = align_up((size_t)n_items * sizeof(HeadsetItem));
  char* dbuf = nullptr;
  if (hipMalloc(&dbuf, b_items + (size_t)n_patches * sizeof(HeadsetPatch) + kAlign) != hipSuccess) {
    (void)hipGetLastError();
    return fail(TVR_ERR_NOMEM, std::string(fn) + ": descriptor buffer");
  }
  hipError_t e = hipMemcpyAsync(dbuf, items, (size_t)n_items * sizeof(HeadsetItem), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && n_patches > 0)
    e = hipMemcpyAsync(dbuf + b_items, patches, (size_t)n_patches * sizeof(HeadsetPatch), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // pageable host memory
  int rc = e == hipSuccess ? TVR_OK : fail(TVR_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  Acts a{resid, nullptr, nullptr, (float*)a2,
         fmt == 0 ? ACT_F32 : fmt == TVR_GEMM_X2F16 ? ACT_X2F16 : fmt == TVR_ACT_X2F16_IL ? ACT_X2F16I : ACT_BF16};
  a.hs_items = (const HeadsetItem*)dbuf;
  a.hs_patches = (const HeadsetPatch*)(dbuf + b_items);
  a.hs_vectors = vectors;
  a.hs_n = n_items;
  a.hs_max_rows = max_rows;
  if (rc == TVR_OK) rc = apply_headset(m, a, st);
  e = hipStreamSynchronize(st);
  if (rc == TVR_OK && e != hipSuccess) rc = fail(TVR_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  (void)hipFree(dbuf);
  return rc;
}

}  // extern "C"
