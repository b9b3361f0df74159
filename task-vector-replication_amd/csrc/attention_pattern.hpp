// attention_pattern.hpp — one query's attention pattern per (sequence, layer, head):
// TransformerLens' blocks.{l}.attn.hook_pattern[0, h, q, :] for one query position q
// per sequence, and optionally its sums over classes of keys ("mass").
//
//   p[j] = softmax_j( rot(Q[q, h]) . rot(K[j, h]) / sqrt(d_head) )   j in [0, q]
//   p[j] = 0                                                          j in (q, ld)
//   mass[c] = sum over j <= q with cls[j] == c of p[j]                (cls -1: nowhere)
//
// Mapping.  ONE wave (a 64-thread block) per (sequence, head), the layer on
// grid.y: every layer of a trace is one launch.  Nothing is accumulated
// against V, so the keys are independent: lane l takes keys l, l + 64, ...,
// reads its key's d_head floats with 16-byte loads, rotates dims
// [0, d_head / 4) (TL rotate-half at the key's absolute position) and dots them
// with the rotated query, which the wave stages once in LDS (every lane reads
// the same address: a broadcast).  The scaled scores stay in LDS, each slot
// written and read by the same lane only; then wave max, expf, wave sum, one
// IEEE division per key and lane-consecutive stores of the row including the
// zeros up to ld.  (attention_row_kernel's form, lanes over dims and the keys
// serial behind a butterfly, pays one shuffle tree per key for nothing here.)
//
// Numerics: fp32 throughout.  The scaled score is rounded once (contraction
// off around the product) and that number enters both the max and the
// exponent, so the best key's weight is exactly exp(0) = 1 (see
// attention_row_kernel).  A key's dot product is four chains (dim e in chain
// e % 4) summed pairwise, every key in the same order: tied keys get equal
// bits.  No atomics; every sum runs in a fixed order — a
// lane's keys in key order, then the xor butterfly 32, 16, .., 1, whose two
// operands commute, so all lanes hold the same bits — which depends on the
// inputs alone, never on the launch geometry.  The mass is computed from the
// normalised p after the pattern is final: asking for it cannot change the
// pattern's bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace tvr {

// sequence s: positions 0 .. qpos at rows row0 .. of the Q | K | V buffer
struct PatternSeq {
  int32_t row0, qpos;
};

constexpr int PATTERN_MAX_CLASSES = 64;

// dynamic LDS of one block: the rotated query and one score per key
inline size_t pattern_lds_bytes(int d_head, int max_keys) { return ((size_t)d_head + (size_t)max_keys) * sizeof(float); }

__device__ __forceinline__ float pattern_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float pattern_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (n_seq * n_heads, n_layers), block 64, dynamic LDS pattern_lds_bytes(DH, longest qpos + 1).
// qkv [layer][row][ldq] with Q | K | V at columns 0 | d | 2 d (before rotary), 16-byte aligned, as the
// tables [n_ctx][DH / 4].  out_pattern [n_seq][n_layers][n_heads][ld] or null; out_mass
// [n_seq][n_layers][n_heads][n_classes] or null (then cls [row] is not read).
template <int DH>
__global__ void __launch_bounds__(64)
attention_pattern_kernel(const float* __restrict__ qkv, size_t layer_stride, int ldq,
                         const PatternSeq* __restrict__ seqs, int n_heads, const int32_t* __restrict__ cls,
                         int n_classes, float* __restrict__ out_pattern, int ld, float* __restrict__ out_mass,
                         const float* __restrict__ cos_t, const float* __restrict__ sin_t, int d, float inv_attn_scale) {
  constexpr int rd = DH / 4, half = rd / 2;
  constexpr int NCH = DH == 16 ? 1 : 3, CH = (DH - rd) / 4 / NCH;  // 16: 1 x 3, 64: 3 x 4, 80: 3 x 5, 128: 3 x 8
  static_assert(DH % 16 == 0 && rd % 4 == 0 && NCH * CH * 4 == DH - rd, "16-byte loads of the rotary and the plain dims");
  using f4 = __attribute__((ext_vector_type(4))) float;
  extern __shared__ __attribute__((aligned(16))) float pattern_lds[];
  float* qs = pattern_lds;       // [DH] the rotated query
  float* sc = pattern_lds + DH;  // [qpos + 1] scores, then exponentials, then probabilities (slot j: lane j % 64 only)
  const int lane = threadIdx.x;
  const int s = blockIdx.x / n_heads, h = blockIdx.x % n_heads, l = blockIdx.y;
  const PatternSeq sd = seqs[s];
  const int nk = sd.qpos + 1;
  const float* base = qkv + (size_t)l * layer_stride + (size_t)sd.row0 * ldq + h * DH;

  {
    const float* qrow = base + (size_t)sd.qpos * ldq;
    for (int i = lane; i < DH; i += 64) {
      float x = qrow[i];
      if (i < rd) {  // x0 cos - x1 sin | x1 cos + x0 sin
        const float p = qrow[i < half ? i + half : i - half];
        const float sg = i < half ? -1.f : 1.f;
        x = x * cos_t[sd.qpos * rd + i] + sg * p * sin_t[sd.qpos * rd + i];
      }
      qs[i] = x;
    }
  }
  __syncthreads();

  float m = -INFINITY;
  for (int j = lane; j < nk; j += 64) {
    const float* kr = base + d + (size_t)j * ldq;
    // four partial dot products, dim e in chain e % 4, summed as (a0 + a1) + (a2 + a3): chains of d_head / 4
    // terms.  One serial chain of 128 (80) fmas measured 1.13 (0.995) of the tests' bar on random scores with
    // 4 x the usual gain; four chains measure at most 0.51 of it (and the fmas of a 16-byte load are independent).
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
    // the plain dims in NCH batches of CH 16-byte loads: a batch's loads are in flight together, and the
    // registers of one batch, not of the whole key, set the occupancy (fully unrolled, d_head 128 took 256)
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

  const size_t slot = ((size_t)s * gridDim.y + l) * n_heads + h;
  float* prow = out_pattern ? out_pattern + slot * ld : nullptr;
  for (int j = lane; j < nk; j += 64) {
    const float p = sc[j] / sum;  // IEEE division: Q = 0 gives fl(1 / fl(q + 1)) bit for bit
    sc[j] = p;
    if (prow) prow[j] = p;
  }
  if (prow)
    for (int j = nk + lane; j < ld; j += 64) prow[j] = 0.f;

  if (out_mass) {
    const int32_t* crow = cls + sd.row0;
    for (int c = 0; c < n_classes; ++c) {
      float a = 0.f;
      for (int j = lane; j < nk; j += 64)
        if (crow[j] == c) a += sc[j];
      a = pattern_wave_sum(a);
      if (lane == 0) out_mass[slot * n_classes + c] = a;
    }
  }
}

}  // namespace tvr
