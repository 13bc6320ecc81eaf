// NIQE of unpaired results: the device part (glare_amd.metrics.niqe; include/glare_hip.h "NIQE of unpaired results").
//
// The score of Mittal, Soundararajan and Bovik ("Making a 'Completely Blind' Image Quality Analyzer", IEEE SPL 2013) as basicsr's
// calculate_niqe evaluates it (driver: defor_cuda_ext/basicsr/metrics/calculate_niqe.py): luma, cropped to whole 96 x 96 blocks; at two
// scales the mean-subtracted contrast-normalised image n, and per block the moments of n and of its four neighbour products, from which
// the host fits the generalised Gaussians.  Four streaming kernels, all fp32 in and out except the fp64 moments:
//   niqe_luma_kernel     uint8 RGB -> integer luma, exact (integer arithmetic, ties to even); four pixels per thread, one 16-byte store
//   niqe_mscn_kernel     a 64 x 16 tile with a 3-pixel replicated halo in LDS; a thread forms four vertically adjacent outputs from a
//                        10 x 7 patch (70 LDS reads instead of 196).  The local moments are taken about the centre pixel c, d = y - c:
//                        E[y^2] - mu^2 in fp32 loses 255^2 * 2^-24 = 0.004 to cancellation, which on a flat region is the whole variance;
//                        S2 - S1^2 of the differences has the error of the differences.
//   niqe_moments_kernel  one workgroup per block, the block in LDS (96 x 96 fp32 = 36 KB); the circular in-block shifts are LDS reads;
//                        products, squares and sums in fp64; lanes add their strided elements in ascending order, a wave butterfly and
//                        four wave partials added in wave order close the sum.
//   niqe_halve_kernel    the 8-tap antialiased bicubic half-size filter: a 32 x 8 output tile, its 22 x 70 reflected input tile in LDS,
//                        the H pass into LDS, then the W pass.
// No atomics, no workspace, every sum in one fixed order: the same bits on every run.  Compiled with -ffp-contract=off: each fmaf below
// is spelt, and the error bounds of tests/test_gpu_niqe_kernels.py count these roundings.
#include "common.h"

namespace {

constexpr int NQ_THREADS = 256;
constexpr int NQ_TW = 64, NQ_TH = 16, NQ_R = 3;                 // mscn: output tile and halo
constexpr int NQ_LW = NQ_TW + 2 * NQ_R, NQ_LH = NQ_TH + 2 * NQ_R;
constexpr int NQ_ROWS = 4;                                      // mscn: outputs per thread, vertically adjacent
constexpr int NQ_HW = 32, NQ_HH = 8;                            // halve: output tile; its input tile is NQ_LH x NQ_LW as well
constexpr int NQ_MAPS = 5, NQ_STATS = 5;
static_assert(2 * NQ_HW + 6 == NQ_LW && 2 * NQ_HH + 6 == NQ_LH, "the halve kernel's input tile");
static_assert(NQ_TW * NQ_TH == NQ_THREADS * NQ_ROWS && NQ_HW * NQ_HH == NQ_THREADS, "one tile per workgroup");

struct NiqeWindow {
  float w[49];
  float s0, oms0;
};

__device__ __forceinline__ float luma_of(int r, int g, int b) {
  const int num = 65481 * r + 128553 * g + 24966 * b;           // <= 55 845 000
  int q = num / 255000;
  const int rem = num - q * 255000;
  q += (rem > 127500 || (rem == 127500 && (q & 1))) ? 1 : 0;    // 16 + q is even exactly when q is
  return (float)(16 + q);
}

__global__ __launch_bounds__(NQ_THREADS) void niqe_luma_kernel(const unsigned char* __restrict__ img, int h, int w, int H, int W,
                                                               float* __restrict__ out) {
  const int W4 = W >> 2;
  const long long q = (long long)blockIdx.x * NQ_THREADS + threadIdx.x;
  if (q >= (long long)H * W4) return;
  const int b = blockIdx.y;
  const int y = (int)(q / W4), x = (int)(q - (long long)y * W4) * 4;
  const unsigned char* p = img + (((size_t)b * h + y) * (size_t)w + x) * 3;
  f32x4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = luma_of(p[3 * k], p[3 * k + 1], p[3 * k + 2]);
  *reinterpret_cast<f32x4*>(out + ((size_t)b * H + y) * (size_t)W + x) = v;
}

__global__ __launch_bounds__(NQ_THREADS) void niqe_mscn_kernel(const float* __restrict__ y, int H, int W, NiqeWindow win,
                                                               float* __restrict__ out) {
  __shared__ float tile[NQ_LH][NQ_LW];
  const int x0 = blockIdx.x * NQ_TW, y0 = blockIdx.y * NQ_TH;
  const float* src = y + (size_t)blockIdx.z * H * W;
  for (int i = threadIdx.x; i < NQ_LH * NQ_LW; i += NQ_THREADS) {
    const int r = i / NQ_LW, c = i - r * NQ_LW;
    const int gy = min(max(y0 - NQ_R + r, 0), H - 1), gx = min(max(x0 - NQ_R + c, 0), W - 1);     // mode = 'nearest'
    tile[r][c] = src[(size_t)gy * W + gx];
  }
  __syncthreads();
  const int tx = threadIdx.x & (NQ_TW - 1), ty = (threadIdx.x / NQ_TW) * NQ_ROWS;
  float c[NQ_ROWS], S1[NQ_ROWS], S2[NQ_ROWS];
#pragma unroll
  for (int k = 0; k < NQ_ROWS; ++k) {
    c[k] = tile[ty + k + NQ_R][tx + NQ_R];
    S1[k] = 0.f;
    S2[k] = 0.f;
  }
#pragma unroll
  for (int r = 0; r < NQ_ROWS + 6; ++r) {
#pragma unroll
    for (int cc = 0; cc < 7; ++cc) {
      const float v = tile[ty + r][tx + cc];
#pragma unroll
      for (int k = 0; k < NQ_ROWS; ++k) {
        const int a = r - k;                                     // the row of v inside output k's 7 x 7 patch
        if (a >= 0 && a < 7) {
          const float d = v - c[k];
          const float wd = win.w[(6 - a) * 7 + (6 - cc)] * d;    // a convolution: the window is flipped
          S1[k] = S1[k] + wd;
          S2[k] = fmaf(wd, d, S2[k]);
        }
      }
    }
  }
  float* dst = out + (size_t)blockIdx.z * H * W;
#pragma unroll
  for (int k = 0; k < NQ_ROWS; ++k) {
    const int oy = y0 + ty + k, ox = x0 + tx;
    if (oy < H && ox < W) {
      const float num = fmaf(c[k], win.oms0, -S1[k]);                                               // y - mu
      const float var = (S2[k] - S1[k] * S1[k]) + win.oms0 * fmaf(c[k] * c[k], win.s0, 2.f * c[k] * S1[k]);
      dst[(size_t)oy * W + ox] = num / (sqrtf(fabsf(var)) + 1.f);
    }
  }
}

__device__ __forceinline__ int reflect(int i, int L) {           // -1 -> 0, -2 -> 1, L -> L - 1; clamped for the discarded part of an edge tile
  i = i < 0 ? -i - 1 : i;
  i = i >= L ? 2 * L - 1 - i : i;
  return min(max(i, 0), L - 1);
}

__global__ __launch_bounds__(NQ_THREADS) void niqe_halve_kernel(const float* __restrict__ y, int H, int W, float* __restrict__ out) {
  __shared__ float tin[NQ_LH][NQ_LW];
  __shared__ float tmid[NQ_HH][NQ_LW];
  constexpr float tap[8] = {-3.f / 256, -9.f / 256, 29.f / 256, 111.f / 256, 111.f / 256, 29.f / 256, -9.f / 256, -3.f / 256};
  const int OH = H >> 1, OW = W >> 1;
  const int ox0 = blockIdx.x * NQ_HW, oy0 = blockIdx.y * NQ_HH;
  const float* src = y + (size_t)blockIdx.z * H * W;
  for (int i = threadIdx.x; i < NQ_LH * NQ_LW; i += NQ_THREADS) {
    const int r = i / NQ_LW, c = i - r * NQ_LW;
    tin[r][c] = src[(size_t)reflect(2 * oy0 - 3 + r, H) * W + reflect(2 * ox0 - 3 + c, W)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NQ_HH * NQ_LW; i += NQ_THREADS) {                                   // the H pass
    const int r = i / NQ_LW, c = i - r * NQ_LW;
    float t = tap[0] * tin[2 * r][c];
#pragma unroll
    for (int a = 1; a < 8; ++a) t = fmaf(tap[a], tin[2 * r + a][c], t);
    tmid[r][c] = t;
  }
  __syncthreads();
  const int tx = threadIdx.x & (NQ_HW - 1), ty = threadIdx.x / NQ_HW;
  const int ox = ox0 + tx, oy = oy0 + ty;
  if (ox < OW && oy < OH) {                                                                         // the W pass
    float t = tap[0] * tmid[ty][2 * tx];
#pragma unroll
    for (int a = 1; a < 8; ++a) t = fmaf(tap[a], tmid[ty][2 * tx + a], t);
    out[((size_t)blockIdx.z * OH + oy) * (size_t)OW + ox] = t;
  }
}

__global__ __launch_bounds__(NQ_THREADS) void niqe_moments_kernel(const float* __restrict__ n, int H, int W, int bh, int bw,
                                                                  double* __restrict__ out) {
  __shared__ float blk[GLARE_NIQE_MAX_BLOCK];
  __shared__ double red[NQ_THREADS / GLARE_WAVE][NQ_MAPS * NQ_STATS];
  const int bx = blockIdx.x, by = blockIdx.y, ne = bh * bw;
  const float* src = n + (size_t)blockIdx.z * H * W + (size_t)by * bh * W + (size_t)bx * bw;
  for (int i = threadIdx.x; i < ne; i += NQ_THREADS) {
    const int r = i / bw, c = i - r * bw;
    blk[i] = src[(size_t)r * W + c];
  }
  __syncthreads();
  double acc[NQ_MAPS][NQ_STATS];
#pragma unroll
  for (int m = 0; m < NQ_MAPS; ++m)
#pragma unroll
    for (int s = 0; s < NQ_STATS; ++s) acc[m][s] = 0.0;
  for (int i = threadIdx.x; i < ne; i += NQ_THREADS) {
    const int r = i / bw, c = i - r * bw;
    const int ru = (r == 0 ? bh : r) - 1, cl = (c == 0 ? bw : c) - 1, cr = c == bw - 1 ? 0 : c + 1;   // np.roll: row r - 1, columns c - 1 / c + 1
    const double v = (double)blk[i];
    const double p[NQ_MAPS] = {v, v * (double)blk[r * bw + cl], v * (double)blk[ru * bw + c], v * (double)blk[ru * bw + cl],
                               v * (double)blk[ru * bw + cr]};                                        // exact: 24 x 24 bits
#pragma unroll
    for (int m = 0; m < NQ_MAPS; ++m) {
      const double sq = p[m] * p[m];
      const bool neg = p[m] < 0.0, pos = p[m] > 0.0;
      acc[m][0] = acc[m][0] + (neg ? 1.0 : 0.0);
      acc[m][1] = acc[m][1] + (pos ? 1.0 : 0.0);
      acc[m][2] = acc[m][2] + (neg ? sq : 0.0);
      acc[m][3] = acc[m][3] + (pos ? sq : 0.0);
      acc[m][4] = acc[m][4] + fabs(p[m]);
    }
  }
  const int lane = threadIdx.x & (GLARE_WAVE - 1), wave = threadIdx.x / GLARE_WAVE;
#pragma unroll
  for (int m = 0; m < NQ_MAPS; ++m)
#pragma unroll
    for (int s = 0; s < NQ_STATS; ++s) {
      double a = acc[m][s];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a = a + __shfl_xor(a, o, 64);      // both partners form the same sum: every lane ends with it
      if (lane == 0) red[wave][m * NQ_STATS + s] = a;
    }
  __syncthreads();
  if (threadIdx.x < NQ_MAPS * NQ_STATS) {
    double a = red[0][threadIdx.x];
    for (int wv = 1; wv < NQ_THREADS / GLARE_WAVE; ++wv) a = a + red[wv][threadIdx.x];
    const size_t block = ((size_t)blockIdx.z * gridDim.x + bx) * gridDim.y + by;                     // column-major over the image
    out[block * (NQ_MAPS * NQ_STATS) + threadIdx.x] = a;
  }
}

inline bool finite_f(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" int glare_niqe_luma_u8(const unsigned char* img_hwc, int B, int h, int w, float* y_out, glare_stream_t stream) {
  if (!img_hwc || !y_out || B <= 0 || h < GLARE_NIQE_BLOCK || w < GLARE_NIQE_BLOCK) return GLARE_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(y_out) & 15) return GLARE_ERR_INVALID;
  const int H = h / GLARE_NIQE_BLOCK * GLARE_NIQE_BLOCK, W = w / GLARE_NIQE_BLOCK * GLARE_NIQE_BLOCK;
  const long long quads = (long long)H * (W / 4);
  if (B > 65535 || cdivll(quads, NQ_THREADS) > 0x7fffffffLL) return GLARE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(niqe_luma_kernel, dim3((unsigned)cdivll(quads, NQ_THREADS), (unsigned)B), dim3(NQ_THREADS), 0, (hipStream_t)stream,
                     img_hwc, h, w, H, W, y_out);
  return glare_launch_status();
}

extern "C" int glare_niqe_mscn_f32(const float* y, int B, int H, int W, const float* window_host, float s0, float one_minus_s0,
                                   float* n_out, glare_stream_t stream) {
  if (!y || !n_out || !window_host || B <= 0 || H <= 0 || W <= 0) return GLARE_ERR_INVALID;
  NiqeWindow win;
  for (int i = 0; i < 49; ++i) {
    if (!finite_f(window_host[i])) return GLARE_ERR_INVALID;
    win.w[i] = window_host[i];
  }
  if (!finite_f(s0) || !finite_f(one_minus_s0)) return GLARE_ERR_INVALID;
  win.s0 = s0;
  win.oms0 = one_minus_s0;
  if (B > 65535 || cdiv(H, NQ_TH) > 65535) return GLARE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(niqe_mscn_kernel, dim3((unsigned)cdiv(W, NQ_TW), (unsigned)cdiv(H, NQ_TH), (unsigned)B), dim3(NQ_THREADS), 0,
                     (hipStream_t)stream, y, H, W, win, n_out);
  return glare_launch_status();
}

extern "C" int glare_niqe_block_moments_f32(const float* n, int B, int H, int W, int bh, int bw, double* out, glare_stream_t stream) {
  if (!n || !out || B <= 0 || H <= 0 || W <= 0 || bh <= 0 || bw <= 0 || bh > H || bw > W) return GLARE_ERR_INVALID;
  if (H % bh != 0 || W % bw != 0) return GLARE_ERR_INVALID;
  if ((long long)bh * bw > GLARE_NIQE_MAX_BLOCK || B > 65535 || H / bh > 65535) return GLARE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(niqe_moments_kernel, dim3((unsigned)(W / bw), (unsigned)(H / bh), (unsigned)B), dim3(NQ_THREADS), 0,
                     (hipStream_t)stream, n, H, W, bh, bw, out);
  return glare_launch_status();
}

extern "C" int glare_niqe_halve_f32(const float* y, int B, int H, int W, float* out, glare_stream_t stream) {
  if (!y || !out || B <= 0 || H < 4 || W < 4 || (H & 1) || (W & 1)) return GLARE_ERR_INVALID;
  if (B > 65535 || cdiv(H / 2, NQ_HH) > 65535) return GLARE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(niqe_halve_kernel, dim3((unsigned)cdiv(W / 2, NQ_HW), (unsigned)cdiv(H / 2, NQ_HH), (unsigned)B), dim3(NQ_THREADS), 0,
                     (hipStream_t)stream, y, H, W, out);
  return glare_launch_status();
}
