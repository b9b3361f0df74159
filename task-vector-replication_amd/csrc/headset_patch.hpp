// headset_patch.hpp — joint head-set patching (TVR_SITE_REPLACE_HEADSET_ALLPOS /
// _LASTPOS): blocks.{l}.attn.hook_result[0, rows, h, :] = v for a SET of (h, v)
// at layer l, applied between the attention and the O + MLP-out GEMM.
//
// With the parallel residual, resid_post = resid_pre + sum_h z_h W_O[h] + b_O
// + mlp_out, and hook_result[h] = z_h W_O[h].  Replacing head h's result by v
// is therefore
//     z_h := 0   in the GEMM's z operand (the head's d_head columns of a2), and
//     resid_pre += v   in the rows the EPI_RESID epilogue accumulates into,
// for ANY v (no solve against W_O[h]).  LayerNorm has read resid_pre by then
// and attention never reads it, so both edits are safe at that point.
//
// One launch per layer that has patches.  Work item: one (site, layer) record;
// its heads are a range of the flat patch list.  grid = (items, row chunks of
// HEADSET_ROWS); every thread of a block handles all the item's heads, the
// vectors are summed in registers in list order and each residual element is
// read and written once: no atomics, fixed order, bitwise reproducible.
//
// The head slices of a2 are addressed in bytes so one kernel serves every
// activation format (split.hpp): a row is `row_bytes` long and holds
// `n_planes` planes `plane_bytes` apart, head h's slice of a plane is
// `slice_bytes` at h * slice_bytes (fp32: 4 d_head, one plane; x2f16: 2 d_head,
// two planes; bf16: 2 d_head, one plane).  d_head % 16 == 0 (check_config), so
// every slice is a whole number of 16-byte words, 16-byte aligned.  Zero is
// all-zero bits in each format.  il (ACT_X2F16I, split.hpp): the row is k-tile-interleaved — the 16-byte word
// of plane pl at logical byte offset b of the plane sits at (b / 64) * 128 + b % 64 + 64 pl.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sweep_desc.hpp"  // HeadsetItem, HeadsetPatch

namespace tvr {

constexpr int HEADSET_THREADS = 256;
constexpr int HEADSET_ROWS = 8;  // rows per block: their residual loads precede their stores

// V4: vectors 16-byte aligned and d % 4 == 0 (float4 residual / vector accesses), else element-wise
// (a caller's offset view of `vectors`; resid itself is always a 256-byte aligned carve).
template <bool V4>
__global__ void __launch_bounds__(HEADSET_THREADS)
headset_patch_kernel(const HeadsetItem* __restrict__ items, const HeadsetPatch* __restrict__ patches,
                     const float* __restrict__ vectors, char* __restrict__ a2, size_t row_bytes, int slice_bytes,
                     int n_planes, size_t plane_bytes, float* __restrict__ resid, int d, int il = 0) {
  const HeadsetItem it = items[blockIdx.x];
  const int r0 = blockIdx.y * HEADSET_ROWS;
  if (r0 >= it.n_rows) return;
  const int nr = min(HEADSET_ROWS, it.n_rows - r0);
  const HeadsetPatch* ps = patches + it.first_patch;

  // zero the listed heads' slices of the z operand
  const int w16 = slice_bytes >> 4, per_head = n_planes * w16, per_row = it.n_patches * per_head;
  for (int x = threadIdx.x; x < nr * per_row; x += HEADSET_THREADS) {
    const int r = x / per_row, y = x - r * per_row;
    const int p = y / per_head, w = y - p * per_head;
    const int pl = w / w16, q = w - pl * w16;
    const size_t b = (size_t)ps[p].head * slice_bytes + (size_t)q * 16;  // byte offset within the plane
    char* dst = a2 + (size_t)(it.row0 + r0 + r) * row_bytes +
                (il ? (b >> 6) * 128 + (b & 63) + (size_t)pl * 64 : (size_t)pl * plane_bytes + b);
    *(uint4*)dst = make_uint4(0u, 0u, 0u, 0u);
  }

  // resid rows += sum of the listed vectors (list order)
  float* rbase = resid + (size_t)(it.row0 + r0) * d;
  if constexpr (V4) {
    for (int c = threadIdx.x; c < d / 4; c += HEADSET_THREADS) {
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int p = 0; p < it.n_patches; ++p) {
        const float4 v = ((const float4*)(vectors + (size_t)ps[p].vec * d))[c];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
      float4 x[HEADSET_ROWS];
#pragma unroll
      for (int u = 0; u < HEADSET_ROWS; ++u) x[u] = ((const float4*)(rbase + (size_t)min(u, nr - 1) * d))[c];
#pragma unroll
      for (int u = 0; u < HEADSET_ROWS; ++u)
        if (u < nr)
          ((float4*)(rbase + (size_t)u * d))[c] = make_float4(x[u].x + s.x, x[u].y + s.y, x[u].z + s.z, x[u].w + s.w);
    }
  } else {
    for (int c = threadIdx.x; c < d; c += HEADSET_THREADS) {
      float s = 0.f;
      for (int p = 0; p < it.n_patches; ++p) s += vectors[(size_t)ps[p].vec * d + c];
      for (int u = 0; u < nr; ++u) rbase[(size_t)u * d + c] += s;
    }
  }
}

}  // namespace tvr
