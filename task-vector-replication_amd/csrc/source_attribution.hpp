// source_attribution.hpp — per-source-token logit attribution of every head from a clean trace: from
// which keys a head carries the answer's logit (the product of attention_pattern.hpp's pattern and
// logit_attribution.hpp's head attribution).
//
// In the processed model b_V = 0 (fold_value_biases), so z[q, h] = sum_j p[j] v[j, h] and, with
// dirs[s] = u_s / sigma_s (attr_direction_kernel),
//   src[s][l][h][j] = p_l,h[q, j] * ((v_l[j, h] @ W_O[l][h]) . dirs[s])          j in [0, q]
//   src[s][l][h][j] = 0                                                          j in (q, ld)
//   cls[s][l][h][c] = sum over j <= q with class[j] == c of src[s][l][h][j]      (class -1: nowhere)
//   sum_j src[s][l][h][j] = out_head[s][l][h] of tvr_trace_logit_attribution
//
// v_j @ W_O[h] . dirs = v_j[h] . g with g[s][h dh + k] = sum_c dirs[s][c] W_O[l][c][h dh + k]: the G = dirs W_O
// of logit_attribution.hpp's head pass.  Two kernels:
//
// head_direction_kernel<NT> — the G pass alone, G[lz][i][d] (fp32) for layers layer0 + lz.  Geometry and
// arithmetic of head_attribution_kernel (its MFMA tile code is repeated here, so that kernel's instruction
// order cannot change): one block of ATTR_WAVES waves per (chunk of ATTR_CHUNK rows, head, layer) on
// v_mfma_f32_16x16x4_f32, K split over the waves in groups of 16 weight rows, the waves' partial tiles summed
// in wave order through LDS.  The MFMA is bit for bit a k-ordered fmaf chain per output element, so the bits
// of G[i][col] depend only on row i of dirs, the layer and the column.  Rows of a short last chunk are masked
// (zero A, no store), not read.
//
// source_attribution_kernel<DH> — ONE wave per (sequence, head), the layer on grid.y, lanes over keys, as
// attention_pattern_kernel, whose pattern it recomputes with that kernel's arithmetic (the same rotary, four
// chains per dot product, the score rounded once, IEEE division: the same bits).  After the normalisation (the
// K pass's registers are free again) lane j reads its key's V slice with 16-byte loads in the pattern kernel's
// batches, dots it with g — staged once in LDS next to the rotated query, read back as a broadcast — on four
// chains (dim e in chain e % 4) summed (a0 + a1) + (a2 + a3), forms c = p * dot as one rounded product and
// stores it.  The class sums are computed from the stored c values, a lane's keys in key order, then the fixed
// xor butterfly: asking for them cannot change out_src's bits.  No atomics; the bits of a (s, l, h) row
// depend on its own inputs alone, not on n_seq or the grid.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "attention_pattern.hpp"
#include "logit_attribution.hpp"

namespace tvr {

// tvr_trace_source_attribution runs the G pass and the source kernel in groups of layers whose [layers][n_seq][d]
// G buffer stays within this many bytes of workspace (one layer at least): every block depends on its own
// (sequence, layer, head) alone, so the grouping cannot change a bit.
constexpr size_t SOURCE_G_CAP_BYTES = (size_t)64 << 20;

// dynamic LDS of one source block: the rotated query, the head's slice of g and one value per key
inline size_t source_lds_bytes(int d_head, int max_keys) {
  return (2 * (size_t)d_head + (size_t)max_keys) * sizeof(float);
}

// out_g[(lz * n + i) * d + h dh + k] = sum_c dirs[i][c] W_O[layer0 + lz][c][h dh + k], i in [0, n), lz = blockIdx.z.
//   dirs   [n][d] dense, 16-B aligned rows
//   w2s    per layer the fp32 [d][ldw2] matrix whose columns [0, d) are W_O (O(head, d_head) order)
// grid (chunks of ATTR_CHUNK rows, H, layers), block 64 * ATTR_WAVES.  NT = d_head / 16.
template <int NT>
__global__ void __launch_bounds__(64 * ATTR_WAVES)
head_direction_kernel(const float* __restrict__ dirs, int n, const float* const* __restrict__ w2s, int layer0,
                      int ldw2, float* __restrict__ out_g, int d) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  constexpr int DH = NT * 16;
  __shared__ float G[ATTR_WAVES][ATTR_CHUNK][DH + 1];
  const int i0 = blockIdx.x * ATTR_CHUNK, h = blockIdx.y, lz = blockIdx.z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r16 = lane & 15, g = lane >> 4;
  const bool live = i0 + r16 < n;
  const float* arow = dirs + (size_t)(live ? i0 + r16 : 0) * d;
  const float* w = w2s[layer0 + lz] + (size_t)h * DH + r16;
  const int ng = d >> 4;  // groups of 16 weight rows
  const int g0 = ng * wave / ATTR_WAVES, g1 = ng * (wave + 1) / ATTR_WAVES;
  f4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
  for (int kg = g0; kg < g1; ++kg) {
    const int k = kg * 16 + 4 * g;
    const float4 a = live ? *(const float4*)(arow + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float aj[4] = {a.x, a.y, a.z, a.w};
    const float* wk = w + (size_t)k * ldw2;
    float b[4][NT];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < NT; ++t) b[j][t] = wk[(size_t)j * ldw2 + t * 16];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aj[j], b[j][t], acc[t], 0, 0, 0);
  }
  // C / D map of the 16 x 16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) G[wave][g * 4 + r][t * 16 + r16] = acc[t][r];
  __syncthreads();
  // the chunk's [16][DH] tile, columns over consecutive threads; the waves' partials in wave order
  float* orow = out_g + ((size_t)lz * n + i0) * d + (size_t)h * DH;
  for (int e = threadIdx.x; e < ATTR_CHUNK * DH; e += 64 * ATTR_WAVES) {
    const int r = e / DH, c = e % DH;
    if (i0 + r >= n) break;  // (rows ascend with e)
    float gs = G[0][r][c];
#pragma unroll
    for (int v = 1; v < ATTR_WAVES; ++v) gs += G[v][r][c];
    orow[(size_t)r * d + c] = gs;
  }
}

// grid (n_seq * n_heads, n_layers), block 64, dynamic LDS source_lds_bytes(DH, longest qpos + 1).
// qkv [layer][row][ldq] with Q | K | V at columns 0 | d | 2 d (before rotary), 16-byte aligned, as the
// tables [n_ctx][DH / 4].  g [layer][n_seq][d] (layer stride g_lstride floats).  Slot of block (s, h, l):
// (s * out_layers + layer0 + l) * n_heads + h; out_src [slot][ld] or null, out_cls [slot][n_classes] or null
// (then cls [row] is not read).
template <int DH>
__global__ void __launch_bounds__(64)
source_attribution_kernel(const float* __restrict__ qkv, size_t layer_stride, int ldq,
                          const PatternSeq* __restrict__ seqs, int n_heads, const float* __restrict__ g,
                          size_t g_lstride, const int32_t* __restrict__ cls, int n_classes,
                          float* __restrict__ out_src, int ld, float* __restrict__ out_cls, int layer0,
                          int out_layers, const float* __restrict__ cos_t, const float* __restrict__ sin_t, int d,
                          float inv_attn_scale) {
  constexpr int rd = DH / 4, half = rd / 2;
  constexpr int NCH = DH == 16 ? 1 : 3, CH = (DH - rd) / 4 / NCH;  // as attention_pattern_kernel
  static_assert(DH % 16 == 0 && rd % 4 == 0 && NCH * CH * 4 == DH - rd, "16-byte loads of the rotary and the plain dims");
  using f4 = __attribute__((ext_vector_type(4))) float;
  extern __shared__ __attribute__((aligned(16))) float source_lds[];
  float* qs = source_lds;           // [DH] the rotated query
  float* gs = source_lds + DH;      // [DH] the head's slice of g
  float* sc = source_lds + 2 * DH;  // [qpos + 1] scores, exponentials, probabilities, then c (slot j: lane j % 64 only)
  const int lane = threadIdx.x;
  const int s = blockIdx.x / n_heads, h = blockIdx.x % n_heads, l = blockIdx.y;
  const PatternSeq sd = seqs[s];
  const int nk = sd.qpos + 1;
  const float* base = qkv + (size_t)l * layer_stride + (size_t)sd.row0 * ldq + h * DH;

  {
    const float* qrow = base + (size_t)sd.qpos * ldq;
    const float* grow = g + (size_t)l * g_lstride + (size_t)s * d + h * DH;
    for (int i = lane; i < DH; i += 64) {
      float x = qrow[i];
      if (i < rd) {  // x0 cos - x1 sin | x1 cos + x0 sin
        const float p = qrow[i < half ? i + half : i - half];
        const float sg = i < half ? -1.f : 1.f;
        x = x * cos_t[sd.qpos * rd + i] + sg * p * sin_t[sd.qpos * rd + i];
      }
      qs[i] = x;
      gs[i] = grow[i];
    }
  }
  __syncthreads();

  // ---- the pattern, statement for statement attention_pattern_kernel's
  float m = -INFINITY;
  for (int j = lane; j < nk; j += 64) {
    const float* kr = base + d + (size_t)j * ldq;
    float a4[4] = {0.f, 0.f, 0.f, 0.f};
    {
      float kx[rd], cs[rd], sn[rd];
#pragma unroll
      for (int c = 0; c < rd; c += 4) {
        const f4 kv = *(const f4*)(kr + c), cv = *(const f4*)(cos_t + j * rd + c), sv = *(const f4*)(sin_t + j * rd + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          kx[c + i] = kv[i];
          cs[c + i] = cv[i];
          sn[c + i] = sv[i];
        }
      }
#pragma unroll
      for (int i = 0; i < half; ++i) {
        const float r0 = kx[i] * cs[i] - kx[i + half] * sn[i];
        const float r1 = kx[i + half] * cs[i + half] + kx[i] * sn[i + half];
        a4[i % 4] = fmaf(qs[i], r0, a4[i % 4]);
        a4[(i + half) % 4] = fmaf(qs[i + half], r1, a4[(i + half) % 4]);
      }
    }
#pragma unroll 1
    for (int c0 = rd; c0 < DH; c0 += 4 * CH) {
      f4 kv[CH];
#pragma unroll
      for (int u = 0; u < CH; ++u) kv[u] = *(const f4*)(kr + c0 + 4 * u);
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        const f4 qv = *(const f4*)(qs + c0 + 4 * u);
#pragma unroll
        for (int i = 0; i < 4; ++i) a4[i] = fmaf(qv[i], kv[u][i], a4[i]);
      }
    }
    float acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
    {
      // rounded once: this number enters the max and the exponent (attention_row_kernel)
#pragma clang fp contract(off)
      acc = acc * inv_attn_scale;
    }
    sc[j] = acc;
    m = fmaxf(m, acc);
  }
  m = pattern_wave_max(m);  // key 0 is always seen: finite

  float sum = 0.f;
  for (int j = lane; j < nk; j += 64) {
    const float e = expf(sc[j] - m);
    sc[j] = e;
    sum += e;
  }
  sum = pattern_wave_sum(sum);

  // ---- the V pass: c[j] = p[j] * (v[j, h] . g), after the normalisation
  const size_t slot = ((size_t)s * out_layers + layer0 + l) * n_heads + h;
  float* srow = out_src ? out_src + slot * ld : nullptr;
  for (int j = lane; j < nk; j += 64) {
    const float p = sc[j] / sum;  // IEEE division, as the pattern kernel's
    const float* vr = base + 2 * d + (size_t)j * ldq;
    float a4[4] = {0.f, 0.f, 0.f, 0.f};
    // four batches of d_head / 16 16-byte loads (the pattern kernel's batch size at d_head 64 / 80 / 128) in ONE
    // rolled loop: with the first batch peeled off, as the K pass has its rotary dims, d_head 64 / 80 took 71 /
    // 90 registers and a wave per SIMD; rolled, they take the pattern kernel's 62 / 80
#pragma unroll 1
    for (int c0 = 0; c0 < DH; c0 += rd) {
      f4 vv[rd / 4];
#pragma unroll
      for (int u = 0; u < rd / 4; ++u) vv[u] = *(const f4*)(vr + c0 + 4 * u);
#pragma unroll
      for (int u = 0; u < rd / 4; ++u) {
        const f4 gv = *(const f4*)(gs + c0 + 4 * u);
#pragma unroll
        for (int i = 0; i < 4; ++i) a4[i] = fmaf(gv[i], vv[u][i], a4[i]);
      }
    }
    const float dot = (a4[0] + a4[1]) + (a4[2] + a4[3]);
    float c;
    {
      // one rounded product
#pragma clang fp contract(off)
      c = p * dot;
    }
    sc[j] = c;
    if (srow) srow[j] = c;
  }
  if (srow)
    for (int j = nk + lane; j < ld; j += 64) srow[j] = 0.f;

  if (out_cls) {
    const int32_t* crow = cls + sd.row0;
    for (int c = 0; c < n_classes; ++c) {
      float a = 0.f;
      for (int j = lane; j < nk; j += 64)
        if (crow[j] == c) a += sc[j];
      a = pattern_wave_sum(a);
      if (lane == 0) out_cls[slot * n_classes + c] = a;
    }
  }
}

}  // namespace tvr
