// w_layout.hpp — the row-pair-interleaved layout of one exact fp16 weight plane (gemm_pingpong.hpp WIL).
//
// A plain plane is halves [N][ldw] (K <= ldw, K % 32 == 0).  The interleaved copy pairs rows 2 p and 2 p + 1 and
// interleaves them per k-tile of 32 columns: halves [ceil(N / 2)][ldw / 32][2][32], so per pair and k-tile 64 B of
// the even row, then 64 B of the odd row — one 128-B line.  The wide one-plane tile's weight piece, 16 rows x 64 B
// of one k-tile, is then 8 whole lines instead of 16 half lines.  A pair is 2 ldw halves, so pair c0 / 2 of an even
// row c0 starts at the plain plane's own offset c0 * ldw.  An odd N has a last pair whose odd row does not exist:
// the copy holds it as zeros, so that the tile's row clamp min(n0 + row, N - 1) and a whole pair's lines stay
// inside the allocation.
//
// Plain C++ without HIP (tests/w_layout_check.cpp runs the helpers on the host); the build kernel under hipcc.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TVR_HD __host__ __device__ __forceinline__
#else
#define TVR_HD inline
#endif

namespace tvr {

constexpr int W_IL_KTILE = 64;  // halves from one k-tile of a row pair to the next

// halves of the interleaved copy of a plane of N rows with row stride ldw
TVR_HD size_t w_il_halves(size_t N, size_t ldw) { return (N + 1) / 2 * 2 * ldw; }

// offset (halves) of element (n, k) in the interleaved copy
TVR_HD size_t w_il_offset(size_t n, size_t k, size_t ldw) {
  return (n >> 1) * 2 * ldw + (k >> 5) * W_IL_KTILE + (n & 1) * 32 + (k & 31);
}

// the weight row a tile at column n0 stages for its row `row` (0-255): rows past N repeat row N - 1
TVR_HD int w_tile_row(int n0, int row, int N) { return n0 + row < N - 1 ? n0 + row : N - 1; }

// offset (halves) of the 16-B piece a lane stages: k-tile 0, 8-halve chunk `chunk` (0-3) of weight row wn; k-tile
// kt is W_IL_KTILE * kt further
TVR_HD size_t w_il_stage_offset(int wn, int chunk, int ldw) {
  return (size_t)(wn >> 1) * (2 * ldw) + (wn & 1) * 32 + chunk * 8;
}

#if defined(__HIPCC__)
// one fp16 plane w [N][K] -> out, its interleaved copy (w_il_halves(N, K) halves; the missing partner row of an
// odd N zeroed)
__global__ void weight_plane_il_kernel(const uint16_t* __restrict__ w, uint16_t* __restrict__ out, size_t N, int K) {
  const size_t n = (N + 1) / 2 * 2 * K;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / K, c = i % K;
    out[w_il_offset(r, c, K)] = r < N ? w[i] : (uint16_t)0;
  }
}
#endif

}  // namespace tvr
