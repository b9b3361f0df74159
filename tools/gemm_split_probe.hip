// gemm_split_probe.hip — speed, in-kernel clock and accuracy of the three GEMM
// paths (fp32 MFMA, 3-plane bf16 split, 2-plane fp16 split) at the engine's
// real shapes, each checked against an fp64 reference on sampled rows.
//   hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize -I include -o tools/gemm_split_probe tools/gemm_split_probe.hip
//   (-fno-slp-vectorize as the engine builds: the sliced form's adds stay scalar)
//   tools/gemm_split_probe [f32|x3|x2|x2p|x2pg|x2pt|bf16 ...]   (default: f32 x3 x2 x2p)
//     x2p  = the engine's planar kernel (A pre-split, LDS-DMA, 16x16x32, EPI_BIAS)
//     x2pg = the same with the QKV+MLP-in epilogue (bias, GELU, split-plane stores)
//     x2pt = K-loop anatomy (cycles in vmcnt drain / barrier, waves 0 and 7)
//     bf16 = the planar kernel on one bf16 plane (TVR_GEMM_BF16; its error is the bf16 rounding)
//     x2pp / bf16pp = the phase-split two-group schedule (gemm_pingpong.hpp); bf16 paths last
//     x2ppwxi / x2pp6wxi = x2ppwx / x2pp6wx (one-plane wide two-phase kernel) with A k-tile-interleaved:
//       8-row x 128-B staging pieces instead of 16-row x 64-B (a path may be named more than once: A B A B ...)
//     x2ppwxiw = x2ppwxi with the weight plane row-pair interleaved as well (W pieces of 8 whole lines)
// A is drawn N(0,1) (a LayerNorm output) or GELU(3 N(0,1)) (the MLP-out input:
// many tiny values, which exercises the fp16 residual plane's range).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../task-vector-replication_amd/csrc/gemm_pingpong.hpp"
#include "gemm_planar_probe.hpp"
#include "../task-vector-replication_amd/csrc/gemm_x2f16.hpp"
#include "../task-vector-replication_amd/csrc/gemm_x3bf16.hpp"

using namespace tvr;

__global__ void fill_normal(float* p, size_t n, unsigned seed, float scale, int gelu) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned x = (unsigned)(i * 2654435761u) ^ seed, y = (unsigned)((i >> 32) * 40503u) ^ (seed * 7919u) ^ (unsigned)i;
    x ^= x >> 13; x *= 0x5bd1e995u; x ^= x >> 15; y ^= x; y ^= y >> 13; y *= 0x5bd1e995u; y ^= y >> 15;
    const float u1 = ((x & 0xffffff) + 0.5f) / 16777216.0f, u2 = ((y & 0xffffff) + 0.5f) / 16777216.0f;
    const float v = scale * sqrtf(-2.f * logf(u1)) * cosf(6.2831853f * u2);
    p[i] = gelu ? gelu_erf(v) : v;
  }
}

__global__ void round_f16_kernel(float* p, size_t n) {  // weights exact in fp16 (a Pythia checkpoint's values)
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = (float)(_Float16)p[i];
}

// A [M][K] fp32 -> the k-tile-interleaved x2f16 layout, halves [M][K / 32][2][32] (a row's two planes of one
// k-tile in one 128-B line): the wxi paths' A operand
__global__ void split_act_f16_il_kernel(const float* __restrict__ a, uint16_t* __restrict__ out, size_t M, int K) {
  const size_t n = M * K;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / K;
    const int c = (int)(i % K);
    const SplitF16 h = split_f16(a[i]);
    uint16_t* o = out + r * 2 * K + (size_t)(c >> 5) * 64 + (c & 31);
    o[0] = h.h0;
    o[32] = h.h1;
  }
}

// (the wxiw path's weight plane: weight_plane_il_kernel, csrc/w_layout.hpp through gemm_pingpong.hpp — the engine's)

__global__ void ref64(const float* A, const float* W, const int* rows, int nr, int N, int K, double* out, double* mag) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nr * N) return;
  const int r = idx / N, n = idx % N;
  const float* a = A + (size_t)rows[r] * K;
  const float* w = W + (size_t)n * K;
  double s = 0, m = 0;
  for (int k = 0; k < K; ++k) { s += (double)a[k] * (double)w[k]; m += fabs((double)a[k] * (double)w[k]); }
  out[idx] = s;
  mag[idx] = m;
}

int main(int argc, char** argv) {
  std::vector<std::string> paths;
  for (int i = 1; i < argc; ++i) paths.push_back(argv[i]);
  if (paths.empty()) paths = {"f32", "x3", "x2", "x2p"};
  struct Shape { const char* name; int M, N, K; int gelu; };
  std::vector<Shape> shapes = {{"qkv_mlpin", 90000, 17920, 2560, 0}, {"o_mlpout", 90000, 2560, 12800, 1}};
  for (auto& s : shapes) {
    float *A, *W, *C;
    uint16_t *W3, *W2, *A2, *A2I = nullptr, *W2I = nullptr;
    unsigned *flag, *wmax_bits;
    unsigned long long* stamps;
    const int maxgrid = gemm_grid<TileSmall>(s.M, s.N);
    hipMalloc(&A, sizeof(float) * (size_t)s.M * s.K);
    hipMalloc(&W, sizeof(float) * (size_t)s.N * s.K);
    hipMalloc(&W3, sizeof(uint16_t) * 3 * (size_t)s.N * s.K);
    hipMalloc(&W2, sizeof(uint16_t) * 2 * (size_t)s.N * s.K);
    hipMalloc(&A2, sizeof(uint16_t) * 2 * (size_t)s.M * s.K);
    hipMalloc(&C, sizeof(float) * (size_t)s.M * s.N);
    hipMalloc(&flag, 8);
    hipMalloc(&wmax_bits, 8);
    hipMalloc(&stamps, sizeof(unsigned long long) * 6 * (size_t)maxgrid);
    hipMemset(flag, 0, 8);
    hipMemset(wmax_bits, 0, 8);
    hipLaunchKernelGGL(fill_normal, dim3(8192), dim3(256), 0, 0, A, (size_t)s.M * s.K, 11u, s.gelu ? 3.0f : 1.0f, s.gelu);
    hipLaunchKernelGGL(fill_normal, dim3(8192), dim3(256), 0, 0, W, (size_t)s.N * s.K, 29u, 0.02f, 0);
    bool w16 = false;  // any one-plane-weight path: W exact in fp16 for every path of the run
    for (const auto& p : paths) w16 = w16 || p.find("wx") != std::string::npos;
    if (w16) hipLaunchKernelGGL(round_f16_kernel, dim3(8192), dim3(256), 0, 0, W, (size_t)s.N * s.K);
    hipLaunchKernelGGL(split_planes_kernel, dim3(8192), dim3(256), 0, 0, W, W3, (size_t)s.N * s.K);
    hipLaunchKernelGGL(absmax_kernel, dim3(2048), dim3(256), 0, 0, W, (size_t)s.N * s.K, wmax_bits);
    unsigned wb = 0;
    hipMemcpy(&wb, wmax_bits, 4, hipMemcpyDeviceToHost);
    float wmax;
    std::memcpy(&wmax, &wb, 4);
    const float wscale = x2_weight_scale(wmax);
    hipLaunchKernelGGL(split_planes_f16_kernel, dim3(8192), dim3(256), 0, 0, W, wscale, W2, (size_t)s.N * s.K);
    const float acc_scale = 1.0f / (wscale * X2_ASCALE);
    hipLaunchKernelGGL(split_act_f16_kernel, dim3(8192), dim3(256), 0, 0, A, A2, (size_t)s.M * s.K);
    bool ail = false;  // any interleaved-A path: a second copy of A in that layout
    for (const auto& p : paths) ail = ail || p == "x2ppwxi" || p == "x2pp6wxi" || p == "x2ppwxiw";
    if (ail) {
      hipMalloc(&A2I, sizeof(uint16_t) * 2 * (size_t)s.M * s.K);
      hipLaunchKernelGGL(split_act_f16_il_kernel, dim3(8192), dim3(256), 0, 0, A, A2I, (size_t)s.M, s.K);
      hipMalloc(&W2I, sizeof(uint16_t) * w_il_halves(s.N, s.K));
      hipLaunchKernelGGL(weight_plane_il_kernel, dim3(8192), dim3(256), 0, 0, W2, W2I, (size_t)s.N, s.K);
    }

    // accuracy rows
    const int nr = 64;
    std::vector<int> hrows(nr);
    for (int i = 0; i < nr; ++i) hrows[i] = (int)((i * 1403ll + 17) % s.M);
    int* drows; double *ref, *mag;
    hipMalloc(&drows, nr * sizeof(int)); hipMalloc(&ref, sizeof(double) * nr * s.N); hipMalloc(&mag, sizeof(double) * nr * s.N);
    hipMemcpy(drows, hrows.data(), nr * sizeof(int), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(ref64, dim3((nr * s.N + 255) / 256), dim3(256), 0, 0, A, W, drows, nr, s.N, s.K, ref, mag);
    std::vector<double> hr(nr * s.N), hm(nr * s.N);
    hipMemcpy(hr.data(), ref, hr.size() * 8, hipMemcpyDeviceToHost);
    hipMemcpy(hm.data(), mag, hm.size() * 8, hipMemcpyDeviceToHost);

    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    for (const auto& path : paths) {
      if (path == "bf16" || path.rfind("bf16pp", 0) == 0) {  // one bf16 plane of A and of W (after every x2 path: they share A2 / W2)
        hipLaunchKernelGGL(act_rows_kernel<ACT_BF16>, dim3(8192), dim3(256), 0, 0, A, s.K, A2, s.M, s.K,
                           (unsigned*)nullptr);  // [M][2][K] halves, plane 0 = bf16(A)
        hipLaunchKernelGGL(bf16_plane_kernel, dim3(8192), dim3(256), 0, 0, W, W2, (size_t)s.N * s.K, 0);
      }
      GemmEpi e{}; e.out0 = C; e.ld0 = s.N;
      int grid = 0;
      auto run = [&](bool stamp) {
        GemmEpi ee = e;
        ee.stamps = stamp ? stamps : nullptr;
        if (path == "f32") {
          grid = gemm_grid<TileLarge>(s.M, s.N);
          hipLaunchKernelGGL((gemm_f32_nt_kernel<EPI_BIAS, TileLarge>), dim3(grid), dim3(TileLarge::THREADS), 0, 0,
                             A, s.K, W, s.K, s.M, s.N, s.K, ee);
        } else if (path == "x3") {
          grid = gemm_x3_grid<X3Large>(s.M, s.N);
          hipLaunchKernelGGL((gemm_x3bf16_nt_kernel<EPI_BIAS, X3Large>), dim3(grid), dim3(X3Large::THREADS), 0, 0,
                             A, s.K, W3, s.K, (size_t)s.N * s.K, s.M, s.N, s.K, ee);
        } else if (path == "x2pt") {
          grid = gemm_planar_grid<PlanarLarge>(s.M, s.N);
          hipLaunchKernelGGL((gemm_planar_kernel<EPI_BIAS, PlanarLarge, ACT_X2F16, true, 2>), dim3(grid),
                             dim3(PlanarLarge::THREADS), 0, 0,
                             A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, ee);
        } else if (path == "x2pg") {  // the engine's QKV+MLP-in epilogue: bias, GELU, split planes
          grid = gemm_planar_grid<PlanarLarge>(s.M, s.N);
          GemmEpi eg = ee;
          eg.n_split = (s.N * 3 / 7) & ~3;  // ~3d of 3d + d_mlp
          eg.out1h = (uint16_t*)(C) + eg.n_split;  // reuse C: row stride 2N halves (bytes of the fp32 row)
          eg.ld1h = 2 * s.N;
          eg.ps1h = s.N;
          eg.range_flag = flag;
          hipLaunchKernelGGL((gemm_planar_kernel<EPI_SPLIT_GELU_ACT, PlanarLarge, ACT_X2F16>), dim3(grid), dim3(PlanarLarge::THREADS),
                             0, 0, A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, eg);
        } else if (path == "bf16") {  // bf16 planar: A2 / W2 re-filled with one bf16 plane below
          grid = gemm_planar_grid<PlanarLarge>(s.M, s.N);
          hipLaunchKernelGGL((gemm_planar_kernel<EPI_BIAS, PlanarLarge, ACT_BF16>), dim3(grid), dim3(PlanarLarge::THREADS),
                             0, 0, A2, 2 * s.K, (size_t)s.K, W2, s.K, (size_t)s.N * s.K, 1.0f, s.M, s.N, s.K, ee);
        } else if (path == "x2pp") {  // phase-split two-group schedule (gemm_pingpong.hpp)
          grid = gemm_pingpong_grid(s.M, s.N);
          hipLaunchKernelGGL((gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16>), dim3(grid), dim3(PP_THREADS), 0, 0,
                             A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, ee);
        } else if (path == "x2pp1" || path == "x2pp2" || path == "x2pp3" || path == "x2pp4" || path == "x2pp12" || path == "x2pp13" || path == "x2pp15" || path == "x2pp21") {  // diagnostic variants (21: TVR_PP_PF flipped)
          grid = gemm_pingpong_grid(s.M, s.N);
          auto kp = path == "x2pp1" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 1>
                    : path == "x2pp21" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 21>
                    : path == "x2pp2" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 2>
                    : path == "x2pp4" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 4>
                    : path == "x2pp12" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 12>
                    : path == "x2pp13" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 13>
                    : path == "x2pp15" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 15>
                                      : gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 3>;
          hipLaunchKernelGGL(kp, dim3(grid), dim3(PP_THREADS), 0, 0,
                             A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, ee);
        } else if (path == "x2ppwx" || path == "x2ppslwx") {  // one-plane (exact fp16) weights, 2 products
          grid = gemm_pingpong_grid(s.M, s.N);
          auto kw = path == "x2ppwx" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 0, false, false, true>
                                     : gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 0, false, true, true>;
          hipLaunchKernelGGL(kw, dim3(grid), dim3(PP_THREADS), 0, 0,
                             A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, ee);
        } else if (path == "x2ppwxw" || path == "x2ppwxn" || path == "x2ppslwxw" || path == "x2ppslwxn" ||
                   path == "x2ppwxw2" || path == "x2ppslwxw2") {
          // one-plane weights on the wide (4 x 2 waves of 64 x 128, VAR 16; two-phase VAR 20) / narrow (pp_tile,
          // VAR 17) wave tile
          grid = gemm_pingpong_grid(s.M, s.N);
          auto kw = path == "x2ppwxw"   ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 16, false, false, true>
                    : path == "x2ppwxn" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 17, false, false, true>
                    : path == "x2ppwxw2" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 20, false, false, true>
                    : path == "x2ppslwxw2" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 20, false, true, true>
                    : path == "x2ppslwxw" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 16, false, true, true>
                                          : gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 17, false, true, true>;
          hipLaunchKernelGGL(kw, dim3(grid), dim3(PP_THREADS), 0, 0,
                             A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, ee);
        } else if (path == "x2ppsl" || path == "x2ppsl14" || path == "x2ppsl13") {  // sliced accumulation (6.9B / 12B)
          grid = gemm_pingpong_grid(s.M, s.N);
          auto ks = path == "x2ppsl" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 0, false, true>
                    : path == "x2ppsl14" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 14, false, true>
                                        : gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 13, false, true>;
          hipLaunchKernelGGL(ks, dim3(grid), dim3(PP_THREADS), 0, 0,
                             A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, ee);
        } else if (path == "x2ppg" || path == "x2ppg7") {  // pingpong with the QKV+MLP-in epilogue, timed
          grid = gemm_pingpong_grid(s.M, s.N);
          GemmEpi eg = ee;
          eg.n_split = (s.N * 3 / 7) & ~255;
          eg.out1h = (uint16_t*)(C) + eg.n_split;
          eg.ld1h = 2 * s.N;
          eg.ps1h = s.N;
          eg.range_flag = flag;
          auto kg = path == "x2ppg" ? gemm_pingpong_kernel<EPI_SPLIT_GELU_ACT, ACT_X2F16, true, 0>
                                    : gemm_pingpong_kernel<EPI_SPLIT_GELU_ACT, ACT_X2F16, true, 7>;
          hipLaunchKernelGGL(kg, dim3(grid), dim3(PP_THREADS),
                             0, 0, A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, eg);
        } else if (path.rfind("x2ppgm", 0) == 0) {  // raster group size: x2ppgm<N>
          grid = gemm_pingpong_grid(s.M, s.N);
          GemmEpi eg = ee;
          eg.group_m = std::stoi(path.substr(6));
          hipLaunchKernelGGL((gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 0>), dim3(grid), dim3(PP_THREADS), 0, 0,
                             A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, eg);
        } else if (path == "x2pp7") {  // register epilogue (EPI_BIAS)
          grid = gemm_pingpong_grid(s.M, s.N);
          hipLaunchKernelGGL((gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 7>), dim3(grid), dim3(PP_THREADS), 0, 0,
                             A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, ee);
        } else if (path == "x2pp8") {  // anatomy with the epilogue's global stores skipped
          grid = gemm_pingpong_grid(s.M, s.N);
          hipLaunchKernelGGL((gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 8>), dim3(grid), dim3(PP_THREADS), 0, 0,
                             A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, ee);
        } else if (path == "bf16pp6") {  // anatomy of the bf16 kernel (pp_tile; one plane each, BK 64)
          grid = gemm_pingpong_grid(s.M, s.N);
          GemmEpi eg = ee;
          hipLaunchKernelGGL((gemm_pingpong_kernel<EPI_BIAS, ACT_BF16, true, 6>), dim3(grid), dim3(PP_THREADS), 0, 0,
                             A2, 2 * s.K, (size_t)s.K, W2, s.K, (size_t)s.N * s.K, 1.0f, s.M, s.N, s.K, eg);
        } else if (path == "x2ppwxi" || path == "x2pp6wxi") {  // interleaved A (row stride 2 K halves), timed / anatomy
          grid = gemm_pingpong_grid(s.M, s.N);
          auto ki = path == "x2ppwxi" ? gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 0, false, false, true, true>
                                      : gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 6, false, false, true, true>;
          hipLaunchKernelGGL(ki, dim3(grid), dim3(PP_THREADS), 0, 0,
                             A2I, 2 * s.K, (size_t)0, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, ee);
        } else if (path == "x2ppwxiw") {  // interleaved A and row-pair interleaved W
          grid = gemm_pingpong_grid(s.M, s.N);
          hipLaunchKernelGGL((gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 0, false, false, true, true, true>),
                             dim3(grid), dim3(PP_THREADS), 0, 0, A2I, 2 * s.K, (size_t)0, W2I, s.K, (size_t)s.N * s.K,
                             acc_scale, s.M, s.N, s.K, ee);
        } else if (path == "x2pp6wx" || path == "x2pp6gwx") {  // anatomy of the one-plane (wide) kernel
          grid = gemm_pingpong_grid(s.M, s.N);
          GemmEpi eg = ee;
          if (path == "x2pp6gwx") {
            eg.n_split = (s.N * 3 / 7) & ~255;
            eg.out1h = (uint16_t*)(C) + eg.n_split;
            eg.ld1h = 2 * s.N;
            eg.ps1h = s.N;
            eg.range_flag = flag;
            hipLaunchKernelGGL((gemm_pingpong_kernel<EPI_SPLIT_GELU_ACT, ACT_X2F16, true, 6, false, false, true>),
                               dim3(grid), dim3(PP_THREADS), 0, 0, A2, s.K, (size_t)s.M * s.K, W2, s.K,
                               (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, eg);
          } else {
            hipLaunchKernelGGL((gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 6, false, false, true>), dim3(grid),
                               dim3(PP_THREADS), 0, 0, A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K,
                               acc_scale, s.M, s.N, s.K, eg);
          }
        } else if (path == "x2pp6" || path == "x2pp6g") {  // per-block anatomy (prologue / loop / epilogue)
          grid = gemm_pingpong_grid(s.M, s.N);
          GemmEpi eg = ee;
          if (path == "x2pp6g") {
            eg.n_split = (s.N * 3 / 7) & ~3;
            eg.out1h = (uint16_t*)(C) + eg.n_split;
            eg.ld1h = 2 * s.N;
            eg.ps1h = s.N;
            eg.range_flag = flag;
            hipLaunchKernelGGL((gemm_pingpong_kernel<EPI_SPLIT_GELU_ACT, ACT_X2F16, true, 6>), dim3(grid), dim3(PP_THREADS),
                               0, 0, A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, eg);
          } else {
            hipLaunchKernelGGL((gemm_pingpong_kernel<EPI_BIAS, ACT_X2F16, true, 6>), dim3(grid), dim3(PP_THREADS), 0, 0,
                               A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, eg);
          }
        } else if (path == "bf16pp" || path == "bf16ppw" || path == "bf16ppn" || path == "bf16ppf") {
          // default / wide (VAR 16) / pp_tile (17) / pp_tile with the q4 prefetch flipped (21, TVR_PP_PF)
          grid = gemm_pingpong_grid(s.M, s.N);
          auto kb = path == "bf16ppw"   ? gemm_pingpong_kernel<EPI_BIAS, ACT_BF16, true, 16>
                    : path == "bf16ppn" ? gemm_pingpong_kernel<EPI_BIAS, ACT_BF16, true, 17>
                    : path == "bf16ppf" ? gemm_pingpong_kernel<EPI_BIAS, ACT_BF16, true, 21>
                                        : gemm_pingpong_kernel<EPI_BIAS, ACT_BF16, true, 0>;
          hipLaunchKernelGGL(kb, dim3(grid), dim3(PP_THREADS), 0, 0,
                             A2, 2 * s.K, (size_t)s.K, W2, s.K, (size_t)s.N * s.K, 1.0f, s.M, s.N, s.K, ee);
        } else if (path == "x2ps") {  // the 128x128 / 4-wave tile at the same shape (2 blocks per CU)
          grid = gemm_planar_grid<PlanarSmall>(s.M, s.N);
          hipLaunchKernelGGL((gemm_planar_kernel<EPI_BIAS, PlanarSmall, ACT_X2F16>), dim3(grid), dim3(PlanarSmall::THREADS), 0, 0,
                             A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, ee);
        } else if (path == "x2p") {
          grid = gemm_planar_grid<PlanarLarge>(s.M, s.N);
          hipLaunchKernelGGL((gemm_planar_kernel<EPI_BIAS, PlanarLarge, ACT_X2F16>), dim3(grid), dim3(PlanarLarge::THREADS), 0, 0,
                             A2, s.K, (size_t)s.M * s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, s.M, s.N, s.K, ee);
        } else {
          grid = gemm_x2_grid<X2Large>(s.M, s.N);
          hipLaunchKernelGGL((gemm_x2f16_nt_kernel<EPI_BIAS, X2Large>), dim3(grid), dim3(X2Large::THREADS), 0, 0,
                             A, s.K, W2, s.K, (size_t)s.N * s.K, acc_scale, flag, s.M, s.N, s.K, ee);
        }
      };
      if (path == "x2pp6" || path == "x2pp6g" || path == "x2pp8" || path == "x2pp6wx" || path == "x2pp6gwx" ||
          path == "x2pp6wxi" || path == "bf16pp6") {
        // block anatomy: medians over blocks (cycles)
        for (int i = 0; i < 5; ++i) run(false);
        run(true);
        hipDeviceSynchronize();
        std::vector<unsigned long long> hs(4 * (size_t)grid);
        hipMemcpy(hs.data(), stamps, hs.size() * 8, hipMemcpyDeviceToHost);
        std::vector<double> pro, loop, epi;
        for (int g = 0; g < grid; ++g) {
          pro.push_back((double)(hs[4 * g + 1] - hs[4 * g]));
          loop.push_back((double)(hs[4 * g + 2] - hs[4 * g + 1]));
          epi.push_back((double)(hs[4 * g + 3] - hs[4 * g + 2]));
        }
        std::sort(pro.begin(), pro.end()); std::sort(loop.begin(), loop.end()); std::sort(epi.begin(), epi.end());
        printf("{\"shape\": \"%s\", \"path\": \"%s\", \"prologue_cyc\": %.0f, \"loop_cyc\": %.0f, "
               "\"loop_cyc_per_ktile\": %.1f, \"epilogue_cyc\": %.0f, \"epilogue_p90\": %.0f}\n", s.name, path.c_str(),
               pro[pro.size() / 2], loop[loop.size() / 2], loop[loop.size() / 2] / (s.K / (path == "bf16pp6" ? 64 : 32)),
               epi[epi.size() / 2],
               epi[epi.size() * 9 / 10]);
        fflush(stdout);
        continue;
      }
      if (path == "x2pt") {  // K-loop anatomy: waves 0 and 7, medians over blocks
        run(true);
        hipDeviceSynchronize();
        std::vector<unsigned long long> hs(6 * (size_t)grid);
        hipMemcpy(hs.data(), stamps, hs.size() * 8, hipMemcpyDeviceToHost);
        for (int w = 0; w < 2; ++w) {
          std::vector<double> fv, fb;
          for (int g = 0; g < grid; ++g) {
            const double L = (double)hs[6 * g + 3 * w];
            if (L > 0) { fv.push_back(hs[6 * g + 3 * w + 1] / L); fb.push_back(hs[6 * g + 3 * w + 2] / L); }
          }
          std::sort(fv.begin(), fv.end());
          std::sort(fb.begin(), fb.end());
          printf("{\"shape\": \"%s\", \"path\": \"x2pt\", \"wave\": %d, \"vmcnt_wait_frac\": %.3f, "
                 "\"barrier_wait_frac\": %.3f}\n", s.name, w ? 7 : 0, fv[fv.size() / 2], fb[fb.size() / 2]);
        }
        fflush(stdout);
        continue;
      }
      run(false); hipDeviceSynchronize();
      hipEventRecord(a); run(false); hipEventRecord(b); hipEventSynchronize(b);
      float ms1; hipEventElapsedTime(&ms1, a, b);
      const int reps = std::max(2, (int)(1500.f / ms1));
      for (int i = 0; i < reps; ++i) run(false);
      hipEventRecord(a);
      for (int i = 0; i < reps; ++i) run(false);
      hipEventRecord(b); hipEventSynchronize(b);
      float ms; hipEventElapsedTime(&ms, a, b);
      ms /= reps;
      run(true);  // stamped launch right after the sustained run: clock under load
      hipDeviceSynchronize();
      std::vector<unsigned long long> hs(2 * grid);
      hipMemcpy(hs.data(), stamps, hs.size() * 8, hipMemcpyDeviceToHost);
      std::vector<double> clk;
      for (int g = 0; g < grid; ++g)
        if (hs[2 * g + 1] > 0) clk.push_back((double)hs[2 * g] / (double)hs[2 * g + 1] * 100.0);  // MHz
      std::sort(clk.begin(), clk.end());
      const double mhz = clk.empty() ? 0 : clk[clk.size() / 2];
      run(false); hipDeviceSynchronize();
      double emax = 0, erms = 0;
      std::vector<float> row(s.N);
      for (int i = 0; i < nr; ++i) {
        hipMemcpy(row.data(), C + (size_t)hrows[i] * s.N, s.N * 4, hipMemcpyDeviceToHost);
        for (int n = 0; n < s.N; ++n) {
          const double err = fabs(row[n] - hr[i * s.N + n]) / hm[i * s.N + n];
          emax = std::max(emax, err);
          erms += err * err;
        }
      }
      unsigned hflag = 0;
      hipMemcpy(&hflag, flag, 4, hipMemcpyDeviceToHost);
      const double fl = 2.0 * s.M * (double)s.N * s.K;
      printf("{\"shape\": \"%s\", \"path\": \"%s\", \"M\": %d, \"N\": %d, \"K\": %d, \"a_dist\": \"%s\", "
             "\"ms\": %.3f, \"tflops\": %.1f, \"clock_mhz\": %.0f, \"err_max\": %.3e, \"err_rms\": %.3e, "
             "\"range_flag\": %u, \"err_unit\": \"|C - C_fp64| / sum_k |a_k w_k|\"}\n",
             s.name, path.c_str(), s.M, s.N, s.K, s.gelu ? "gelu(3N(0,1))" : "N(0,1)", ms, fl / (ms * 1e-3) / 1e12,
             mhz, emax, sqrt(erms / ((double)nr * s.N)), hflag);
      fflush(stdout);
    }
    hipFree(A); hipFree(A2); hipFree(A2I); hipFree(W2I); hipFree(W); hipFree(W3); hipFree(W2); hipFree(C); hipFree(flag); hipFree(wmax_bits);
    hipFree(stamps); hipFree(drows); hipFree(ref); hipFree(mag);
  }
  return 0;
}
