// logit_attribution.hpp — direct logit attribution (DLA) from a clean trace.
//
// TransformerLens: cache.stack_head_results / accumulated_resid -> apply_ln_to_stack -> logit_attrs.  With
// u = W_U'[:, target] - W_U'[:, contrast] and sigma the final LayerNorm's scale of the query row,
//   out_resid[s][l]   = (x_l - mean x_l) . u / sigma          x_l = blocks.{l}.hook_resid_pre[q]  (x_L: final)
//   out_head[s][l][h] = (z_l[q][h] @ W_O[l][h]) . u / sigma
//
// Direction pass (small): attr_direction_kernel, one wave per sequence, writes dirs[s] = u_s / sigma_s;
// attr_resid_kernel, one wave per (sequence, layer), the centred dot.  The row mean is computed as
// center_rows_kernel<true> / resid_capture_partial_kernel<true> compute it (same lane partition and order), so
// the centred values are the ones tvr_trace_read exports.
//
// Head pass (the hot path): per layer G = dirs W_O ([S x d] . [d x d], S sequences), then
// out[s][h] = sum_k z[s][h dh + k] G[s][h dh + k].  Only S FMAs per weight read: the weights' arrival bounds it.
// head_attribution_kernel runs one block per (chunk of 16 sequences, head, layer) on the fp32-input MFMA
// v_mfma_f32_16x16x4_f32: A = a 16 x 4 slice of the chunk's direction rows, B = 4 rows of w2 by 16 of the
// head's z-columns (w2[c][h dh + k] is contiguous in k; d_head % 16 == 0, so a tile never straddles two
// heads).  The K range [0, d) is split over the block's ATTR_WAVES waves in groups of 16 rows; within a group
// the lane quarter g supplies rows 4 g + j at step j (one float4 of the direction row per lane and group).
// The MFMA is bit for bit a k-ordered fmaf chain per output element, so element (i, col) depends on row i of
// dirs and column col of W_O alone.  The waves' partial tiles meet in LDS and are summed in wave order; the z
// dot then runs as four chains over the head's columns (a quarter of d_head each, in column order), summed
// pairwise (p0 + p1) + (p2 + p3).  No atomics; the geometry is fixed, so the bits of out[i][h] depend only on
// row i's inputs, the layer and the head — never on n or the chunk the row lands in.  Rows of a short last
// chunk are masked (zero A, no z read, no store), not read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "split.hpp"

namespace tvr {

constexpr int ATTR_CHUNK = 16;  // sequences per block: the M of the 16 x 16 x 4 MFMA
constexpr int ATTR_WAVES = 4;   // K split of one block (fixed: part of the summation order)

// dirs[s][:] = (W_U'[:, target[s]] - W_U'[:, contrast[s]]) / sigma_s, sigma_s the LNPre scale of row rows[s] of
// the final residual x (sqrt(mean((x - mean x)^2) + eps)).  wu: [V][d] (w_unembed_t), 16-B aligned rows.
__global__ void __launch_bounds__(64)
attr_direction_kernel(const float* __restrict__ x, const int32_t* __restrict__ rows, const float* __restrict__ wu,
                      const int32_t* __restrict__ target, const int32_t* __restrict__ contrast, float eps,
                      float* __restrict__ dirs, int d) {
  const int s = blockIdx.x, lane = threadIdx.x, d4 = d >> 2;
  const float4* xr = (const float4*)(x + (size_t)rows[s] * d);
  float sum = 0.f;
  for (int c = lane; c < d4; c += 64) {
    const float4 v = xr[c];
    sum += (v.x + v.y) + (v.z + v.w);
  }
  const float mean = wave_sum(sum) / (float)d;
  float ss = 0.f;
  for (int c = lane; c < d4; c += 64) {
    float4 v = xr[c];
    v.x -= mean; v.y -= mean; v.z -= mean; v.w -= mean;
    ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
  }
  const float sigma = sqrtf(wave_sum(ss) / (float)d + eps);
  const float4* ut = (const float4*)(wu + (size_t)target[s] * d);
  const float4* uc = contrast ? (const float4*)(wu + (size_t)contrast[s] * d) : nullptr;
  float4* o = (float4*)(dirs + (size_t)s * d);
  for (int c = lane; c < d4; c += 64) {
    float4 u = ut[c];
    if (uc) {
      const float4 w = uc[c];
      u.x -= w.x; u.y -= w.y; u.z -= w.z; u.w -= w.w;
    }
    o[c] = make_float4(u.x / sigma, u.y / sigma, u.z / sigma, u.w / sigma);
  }
}

// out[s][l] = (x_l - mean x_l) . dirs[s], x_l = row rows[s] of slab l of resid (slab stride lstride floats).
// One wave per (sequence, layer): each lane's float4 columns in order on four chains, (a0 + a1) + (a2 + a3),
// then wave_sum.
__global__ void __launch_bounds__(64)
attr_resid_kernel(const float* __restrict__ resid, size_t lstride, const int32_t* __restrict__ rows,
                  const float* __restrict__ dirs, float* __restrict__ out, int n_layers1, int d) {
  const int s = blockIdx.x, l = blockIdx.y, lane = threadIdx.x, d4 = d >> 2;
  const float4* xr = (const float4*)(resid + (size_t)l * lstride + (size_t)rows[s] * d);
  const float4* u = (const float4*)(dirs + (size_t)s * d);
  float sum = 0.f;
  for (int c = lane; c < d4; c += 64) {
    const float4 v = xr[c];
    sum += (v.x + v.y) + (v.z + v.w);
  }
  const float mean = wave_sum(sum) / (float)d;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int c = lane; c < d4; c += 64) {
    const float4 v = xr[c];
    const float4 w = u[c];
    a0 = fmaf(v.x - mean, w.x, a0);
    a1 = fmaf(v.y - mean, w.y, a1);
    a2 = fmaf(v.z - mean, w.z, a2);
    a3 = fmaf(v.w - mean, w.w, a3);
  }
  const float a = wave_sum((a0 + a1) + (a2 + a3));
  if (lane == 0) out[(size_t)s * n_layers1 + l] = a;
}

// out[(i * out_layers + lz) * H + h] = (z_i[h dh ..] @ W_O[layer0 + lz][h]) . dirs[i], i in [0, n), lz = blockIdx.z.
//   dirs   [n][d] dense, 16-B aligned rows
//   z      row (zrows ? zrows[i] : i) of slab lz (slab stride z_lstride floats), rows of d floats
//   w2s    per layer the fp32 [d][ldw2] matrix whose columns [0, d) are W_O (O(head, d_head) order)
// grid (chunks of ATTR_CHUNK rows, H, layers), block 64 * ATTR_WAVES.  NT = d_head / 16.
template <int NT>
__global__ void __launch_bounds__(64 * ATTR_WAVES)
head_attribution_kernel(const float* __restrict__ dirs, int n, const float* __restrict__ z, size_t z_lstride,
                        const int32_t* __restrict__ zrows, const float* const* __restrict__ w2s, int layer0,
                        int ldw2, float* __restrict__ out, int out_layers, int H, int d) {
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
  if (wave != 0) return;
  const int i = i0 + r16;  // lane (row r16, quarter g of the head's columns)
  float p = 0.f;
  if (i < n) {
    const float* zr = z + (size_t)lz * z_lstride + (size_t)(zrows ? zrows[i] : i) * d + (size_t)h * DH;
    for (int c = g * (DH / 4); c < (g + 1) * (DH / 4); ++c) {
      float gs = G[0][r16][c];
#pragma unroll
      for (int v = 1; v < ATTR_WAVES; ++v) gs += G[v][r16][c];
      p = fmaf(zr[c], gs, p);
    }
  }
  p += __shfl_xor(p, 16, 64);
  p += __shfl_xor(p, 32, 64);
  if (g == 0 && i < n) out[((size_t)i * out_layers + lz) * H + h] = p;
}

}  // namespace tvr
