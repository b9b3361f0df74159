// attention_knockout.hpp — attention knockout of a sequence's LAST query: for the listed heads h,
// TransformerLens' blocks.{l}.attn.hook_attn_scores[0, h, -1, j] = -inf for the blocked keys j, i.e.
//
//   p[j] = softmax over the keys j <= q, j not blocked, of rot(Q[q, h]) . rot(K[j, h]) / sqrt(d_head)
//   p[j] = 0 on the blocked keys
//   z[q, h] = sum_j p[j] V[j, h]
//
// and z[q, h] overwrites the slice the attention launch wrote (tvr_patch_sweep_knockout: between the
// attention and the O + MLP-out GEMM, where the head-set patch sits).  Heads that are not listed, other
// rows and the MLP columns of z are not touched.
//
// Mapping.  ONE wave (a 64-thread block) per (item, head); a head outside the item's mask leaves at once.
// Scores as attention_pattern_kernel computes them: lane l takes keys l, l + 64, .., 16-byte loads of the
// key's slice, rotate-half on dims [0, d_head / 4) at the key's position, four fma chains summed pairwise
// against the rotated query in LDS; the scores stay in LDS.  A blocked key is SKIPPED (a select on its bit
// of the item's mask): it has no score, and enters neither the max, the sum nor the product with V — no
// -inf anywhere, so no exp(-inf - -inf).  The host guarantees one unblocked key, so the max is finite and
// the sum at least 1.  Then p = e / sum (IEEE division) in LDS and z = P V with lane l on dims l, l + 64:
// one fma chain per dim over the unblocked keys in key order, V read as 256-byte row runs, four keys'
// loads in flight.  z leaves through LDS as 4-dim groups (store_act4 / act_col: all four formats).
//
// Numerics: fp32; the scaled score is rounded once (contraction off), so the best unblocked key's weight is
// exactly exp(0) = 1 (attention_row_kernel's comment).  Every reduction has a fixed order that depends on
// the sequence, the head and the blocked set alone — a lane's keys in key order, the commutative xor
// butterfly, the key-order chain of P V — never on n_items, the grid or the other items.  No atomics
// (but the x2f16 range flag, which carries no value).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "attention_pattern.hpp"
#include "split.hpp"
#include "sweep_desc.hpp"

namespace tvr {

// dynamic LDS of one block: the rotated query, the z slice and one score per key
inline size_t knockout_lds_bytes(int d_head, int max_keys) {
  return (2 * (size_t)d_head + (size_t)max_keys) * sizeof(float);
}

__device__ __forceinline__ bool knockout_blocked(const uint32_t* __restrict__ mask, int j) {
  return (mask[j >> 5] >> (j & 31)) & 1u;
}

// grid n_items * n_heads, block 64, dynamic LDS knockout_lds_bytes(DH, longest p0 + n).
// qkv [row][ldq] with Q | K | V at columns 0 | d | 2 d (before rotary); positions < p0 of a sequence are
// rows cache_row .. of `cache` (row stride ldc), or of qkv itself when prefix_live (SeqDesc).  z: the
// activation buffer [rows][ldz] of format FMT (fp32, or halves [rows][2 ldz]).  Tables [n_ctx][DH / 4].
template <int FMT, int DH>
__global__ void __launch_bounds__(64)
attention_knockout_kernel(const float* __restrict__ qkv, int ldq, const float* __restrict__ cache, int ldc,
                          const SeqDesc* __restrict__ seqs, const KnockoutItem* __restrict__ items,
                          const uint32_t* __restrict__ masks, int n_heads, void* __restrict__ z, int ldz,
                          unsigned* __restrict__ flag, const float* __restrict__ cos_t,
                          const float* __restrict__ sin_t, int d, float inv_attn_scale) {
  constexpr int rd = DH / 4, half = rd / 2;
  constexpr int NCH = DH == 16 ? 1 : 3, CH = (DH - rd) / 4 / NCH;  // as attention_pattern_kernel
  constexpr int NDL = (DH + 63) / 64;                             // dims per lane in P V
  constexpr int KB = 4;                                           // keys whose V loads are in flight together
  static_assert(DH % 16 == 0 && DH <= 128 && rd % 4 == 0 && NCH * CH * 4 == DH - rd, "head size");
  using f4 = __attribute__((ext_vector_type(4))) float;
  typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
  extern __shared__ __attribute__((aligned(16))) float knockout_lds[];
  float* qs = knockout_lds;           // [DH] the rotated query
  float* zs = knockout_lds + DH;      // [DH] the z slice
  float* sc = knockout_lds + 2 * DH;  // [T] scores, exponentials, probabilities (slot j: lane j % 64 until the barrier)
  const int lane = threadIdx.x;
  const int item = blockIdx.x / n_heads, h = blockIdx.x % n_heads;
  const KnockoutItem it = items[item];
  if (!(((h < 32 ? it.heads_lo : it.heads_hi) >> (h & 31)) & 1u)) return;  // the whole block
  const SeqDesc sd = seqs[it.seq];
  const uint32_t* mask = masks + it.mask_off;
  const int T = sd.p0 + sd.n, qpos = T - 1;
  const float* pfx = sd.prefix_live ? qkv : cache;
  const int ldp = sd.prefix_live ? ldq : ldc;
  auto row_of = [&](int j) -> const float* {
    return j < sd.p0 ? pfx + (size_t)(sd.cache_row + j) * ldp : qkv + (size_t)(sd.row0 + j - sd.p0) * ldq;
  };

  {
    const float* qrow = row_of(qpos) + h * DH;
    for (int i = lane; i < DH; i += 64) {
      float x = qrow[i];
      if (i < rd) {  // x0 cos - x1 sin | x1 cos + x0 sin
        const float p = qrow[i < half ? i + half : i - half];
        const float sg = i < half ? -1.f : 1.f;
        x = x * cos_t[qpos * rd + i] + sg * p * sin_t[qpos * rd + i];
      }
      qs[i] = x;
    }
  }
  __syncthreads();

  float m = -INFINITY;
  for (int j = lane; j < T; j += 64) {
    if (knockout_blocked(mask, j)) continue;
    const float* kr = row_of(j) + d + h * DH;
    float a4[4] = {0.f, 0.f, 0.f, 0.f};  // dim e in chain e % 4, summed as (a0 + a1) + (a2 + a3)
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
  m = pattern_wave_max(m);  // one key at least is not blocked (checked on the host): finite

  float sum = 0.f;
  for (int j = lane; j < T; j += 64) {
    if (knockout_blocked(mask, j)) continue;
    const float e = expf(sc[j] - m);
    sc[j] = e;
    sum += e;
  }
  sum = pattern_wave_sum(sum);
  for (int j = lane; j < T; j += 64) sc[j] = knockout_blocked(mask, j) ? 0.f : sc[j] / sum;
  __syncthreads();

  // z = P V: lane l owns dims l + 64 u, one chain per dim over the unblocked keys in key order
  float acc[NDL];
#pragma unroll
  for (int u = 0; u < NDL; ++u) acc[u] = 0.f;
  const int vcol = 2 * d + h * DH;
  for (int j0 = 0; j0 < T; j0 += KB) {
    float vv[KB][NDL];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const float* vr = row_of(min(j0 + k, T - 1)) + vcol;
#pragma unroll
      for (int u = 0; u < NDL; ++u) vv[k][u] = lane + 64 * u < DH ? vr[lane + 64 * u] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int j = j0 + k;
      if (j >= T || knockout_blocked(mask, j)) continue;  // block-uniform
      const float p = sc[j];
#pragma unroll
      for (int u = 0; u < NDL; ++u) acc[u] = fmaf(p, vv[k][u], acc[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < NDL; ++u)
    if (lane + 64 * u < DH) zs[lane + 64 * u] = acc[u];
  __syncthreads();

  const size_t zrow = (size_t)(sd.row0 + sd.n - 1);
  for (int c = 4 * lane; c < DH; c += 256) {
    const f4 v = *(const f4*)(zs + c);
    if constexpr (FMT != ACT_F32)
      store_act4<FMT>((uint16_t*)z + zrow * 2 * ldz + act_col<FMT>(h * DH + c), act_ps<FMT>(ldz), v[0], v[1], v[2], v[3], flag);
    else
      *(f4u*)((float*)z + zrow * ldz + h * DH + c) = v;
  }
}

}  // namespace tvr
