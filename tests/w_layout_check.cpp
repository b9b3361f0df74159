// Host-only checks of the row-pair-interleaved weight layout (csrc/w_layout.hpp): the helpers the wide one-plane
// GEMM tile, the layout kernel and the engine's allocation share.  For every (N, K) below and every tile column
// n0, tile row, 16-byte chunk and k-tile, the 8 halves a lane stages lie inside w_il_halves(N, K), and a host
// copy built with w_il_offset read back through the staging formula returns w[n][k] for every real element and
// 0 in the partner row of an odd N.  The copy lives in a heap buffer of exactly the helper's size, so under the
// address sanitizer an offset past it fails on its own.  Built and run by tests/test_w_layout_host.py, plain
// and with the address and undefined-behaviour sanitizers; exits non-zero at the first failed check.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "w_layout.hpp"

using namespace tvr;

namespace {

int g_N = 0, g_K = 0;

#define CHECK(cond)                                                                                       \
  do {                                                                                                    \
    if (!(cond)) {                                                                                        \
      std::fprintf(stderr, "%s:%d: N %d K %d: check failed: %s\n", __FILE__, __LINE__, g_N, g_K, #cond); \
      std::exit(1);                                                                                       \
    }                                                                                                     \
  } while (0)

// a value that names its element (never 0, so the zeroed row is told apart)
uint16_t value(int n, int k) { return (uint16_t)(1 + (n * 2579 + k * 7) % 65521 % 65535); }

long check(int N, int K) {
  g_N = N;
  g_K = K;
  const size_t halves = w_il_halves(N, K);
  CHECK(halves == (size_t)((N + 1) / 2) * 2 * K);
  // the layout kernel's loop on the host: every row of every pair, rows past N as zeros
  std::vector<uint16_t> w((size_t)N * K);
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) w[(size_t)n * K + k] = value(n, k);
  uint16_t* il = (uint16_t*)std::malloc(halves * sizeof(uint16_t));
  CHECK(il != nullptr);
  for (size_t i = 0; i < halves; ++i) il[i] = 0xFFFF;
  std::vector<char> written(halves, 0);
  const int rows = (N + 1) / 2 * 2;
  for (int r = 0; r < rows; ++r)
    for (int k = 0; k < K; ++k) {
      const size_t o = w_il_offset(r, k, K);
      CHECK(o < halves);
      CHECK(!written[o]);  // a bijection onto the allocation
      written[o] = 1;
      il[o] = r < N ? w[(size_t)r * K + k] : (uint16_t)0;
    }
  for (size_t i = 0; i < halves; ++i) CHECK(written[i]);
  // the tile's reads
  long reads = 0;
  for (int n0 = 0; n0 < N; n0 += 256)
    for (int row = 0; row < 256; ++row) {
      const int wn = w_tile_row(n0, row, N);
      CHECK(wn >= 0 && wn < N);
      CHECK(wn == (n0 + row < N ? n0 + row : N - 1));
      for (int chunk = 0; chunk < 4; ++chunk)
        for (int kt = 0; kt < K / 32; ++kt) {
          const size_t o = w_il_stage_offset(wn, chunk, K) + (size_t)kt * W_IL_KTILE;
          CHECK(o % 8 == 0);  // 16-byte pieces
          CHECK(o + 8 <= halves);
          for (int j = 0; j < 8; ++j) CHECK(il[o + j] == w[(size_t)wn * K + kt * 32 + chunk * 8 + j]);
          ++reads;
        }
    }
  // every element through the element formula, and the partner row of an odd N
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) CHECK(il[w_il_offset(n, k, K)] == w[(size_t)n * K + k]);
  if (N & 1)
    for (int k = 0; k < K; ++k) CHECK(il[w_il_offset(N, k, K)] == 0);
  // an even row's pair starts at the row's own offset in the plain plane (the engine's column offsets)
  for (int n = 0; n < N; n += 2) CHECK(w_il_offset(n, 0, K) == (size_t)n * K);
  std::free(il);
  return reads;
}

}  // namespace

int main() {
  const int Ns[] = {1, 2, 7, 255, 256, 257, 258}, Ks[] = {32, 64, 96, 2560};
  long reads = 0;
  for (int N : Ns)
    for (int K : Ks) reads += check(N, K);
  std::printf("w_layout_check: ok (%ld staged pieces)\n", reads);
  return 0;
}
