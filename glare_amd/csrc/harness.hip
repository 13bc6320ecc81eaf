// Pre/post-processing of the inference harness on the device: the steps
// code/infer_dataset_lol.py:113-153 runs per image on the host with numpy / cv2, batched here so that the images cross
// PCIe once as uint8 and only one PSNR per image comes back.
//   pre : reflect-pad 20 px bottom / left (impad, :71-72), /255 (t, :42), log(clamp(x + 1e-3, min = 1e-3)) (:127-128)
//   post: crop [:, :, :h, 20:], clamp [0,1] (:135-140), gain = gray(GT/255) / gray(out) with the cv2.COLOR_BGR2GRAY weights
//         applied to RGB-ordered data, i.e. 0.114 ch0 + 0.587 ch1 + 0.299 ch2 (:142-144), clip, PSNR (utils2.py:32-36)
#include "common.h"

namespace {

constexpr int HB = 64;  // blocks per image of the two-level reductions

__global__ __launch_bounds__(256) void pre_kernel(const uint8_t* __restrict__ img, int B, int H, int W, int pad,
                                                  float* __restrict__ out) {
  const int Hp = H + pad, Wp = W + pad;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)B * 3 * Hp * Wp;
  if (i >= total) return;
  const int x = (int)(i % Wp), y = (int)((i / Wp) % Hp), c = (int)((i / ((long long)Wp * Hp)) % 3), b = (int)(i / ((long long)Wp * Hp * 3));
  // np.pad(..., 'reflect'): the edge is not repeated; pads longer than the image keep reflecting (period 2n - 2)
  const int py = y % (2 * H - 2), px = (x >= pad ? x - pad : pad - x) % (2 * W - 2);
  const int ys = py < H ? py : 2 * H - 2 - py;
  const int xs = px < W ? px : 2 * W - 2 - px;
  const float v = (float)img[(((long long)b * H + ys) * W + xs) * 3 + c];
  out[i] = logf(fmaxf(__fdiv_rn(v, 255.f) + 1e-3f, 1e-3f));
}

// pass 1: r = clamp(crop(out)) -> restored (NHWC), per-block sums of gray(r) and gray(gt/255)
__global__ __launch_bounds__(256) void post_crop_kernel(const float* __restrict__ out, const uint8_t* __restrict__ gt, int h, int w,
                                                        int Hp, int Wp, int pad, float* __restrict__ restored,
                                                        double* __restrict__ partial, int* __restrict__ bad_partial) {
  __shared__ double red[2][4];
  __shared__ int redc[4];
  const int b = blockIdx.y;
  const long long npix = (long long)h * w;
  double sr = 0.0, sg = 0.0;
  int bad = 0;       // non-finite values of the network output inside the crop, counted BEFORE the clamp: the clamp turns +inf into 1.0
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)HB * 256) {
    const int y = (int)(p / w), x = (int)(p % w);
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = out[(((long long)b * 3 + c) * Hp + y) * Wp + x + pad];
      bad += (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;   // exponent all ones: inf or NaN (an fp16 overflow upstream)
      r[c] = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);     // torch.clamp (infer_dataset_lol.py:138): a NaN stays a NaN -- fminf / fmaxf
                                                      // would turn it into 0 and hide a broken image behind a finite PSNR
      restored[((long long)b * npix + p) * 3 + c] = r[c];
    }
    sr += (double)(0.114f * r[0] + 0.587f * r[1] + 0.299f * r[2]);
    if (gt) {
      const uint8_t* g = gt + ((long long)b * npix + p) * 3;
      sg += 0.114 * (g[0] / 255.0) + 0.587 * (g[1] / 255.0) + 0.299 * (g[2] / 255.0);
    }
  }
  for (int o = 32; o > 0; o >>= 1) { sr += __shfl_xor(sr, o, 64); sg += __shfl_xor(sg, o, 64); bad += __shfl_xor(bad, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sr; red[1][threadIdx.x >> 6] = sg; redc[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x < 2)
    partial[((size_t)b * HB + blockIdx.x) * 2 + threadIdx.x] =
        (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
  if (threadIdx.x == 2 && bad_partial) bad_partial[(size_t)b * HB + blockIdx.x] = (redc[0] + redc[1]) + (redc[2] + redc[3]);
}

__global__ void post_count_kernel(const int* __restrict__ bad_partial, int B, int* __restrict__ nonfinite) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int s = 0;
  for (int k = 0; k < HB; ++k) s += bad_partial[(size_t)b * HB + k];
  nonfinite[b] = s;
}

// pass 2: r = clip(r * gain), per-block sum of (gt/255 - r)^2
__global__ __launch_bounds__(256) void post_gain_kernel(float* __restrict__ restored, const uint8_t* __restrict__ gt, long long n,
                                                        const double* __restrict__ partial, int apply_gain,
                                                        double* __restrict__ mse_partial) {
  __shared__ double red[4];
  __shared__ float gain_s;
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    double sr = 0.0, sg = 0.0;
    for (int k = 0; k < HB; ++k) { sr += partial[((size_t)b * HB + k) * 2]; sg += partial[((size_t)b * HB + k) * 2 + 1]; }
    gain_s = apply_gain ? (float)(sg / sr) : 1.f;      // ratio of the two means (same pixel count)
  }
  __syncthreads();
  const float gain = gain_s;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)HB * 256) {
    float r = restored[(long long)b * n + i];
    if (apply_gain) { r *= gain; r = r < 0.f ? 0.f : (r > 1.f ? 1.f : r); }   // np.clip: NaN propagates
    restored[(long long)b * n + i] = r;
    if (gt) {
      const double d = gt[(long long)b * n + i] / 255.0 - (double)r;
      acc += d * d;
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) mse_partial[(size_t)b * HB + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void post_psnr_kernel(const double* __restrict__ mse_partial, long long n, int B, double* __restrict__ psnr) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int k = 0; k < HB; ++k) s += mse_partial[(size_t)b * HB + k];
  const double mse = s / (double)n;
  psnr[b] = mse == 0.0 ? 100.0 : 10.0 * log10(1.0 / mse);
}

// img_as_ubyte of both images as float planes in [0, 255] (the operands of calculate_ssim, infer_dataset_lol.py:152):
// restored float in [0,1] -> rint(clip * 255) (skimage's float -> uint8 conversion rounds to nearest even), the GT as is
__global__ __launch_bounds__(256) void ubyte_planes_kernel(const float* __restrict__ restored, const uint8_t* __restrict__ gt, long long n,
                                                           float* __restrict__ x255, float* __restrict__ y255) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  x255[i] = rintf(fminf(fmaxf(restored[i], 0.f), 1.f) * 255.f);
  y255[i] = (float)gt[i];
}


// ---- unpaired harness (code/infer_unpaired.py:81-136): any size, borders on all four sides, uint8 out --------------------
// cv2.borderInterpolate: REFLECT101 (numpy 'reflect', gfedcb|abcdefgh|gfedcba) folds with period 2n - 2, REFLECT (numpy
// 'symmetric', cv2.BORDER_REFLECT, fedcba|abcdefgh|hgfedcb) with period 2n; a side of one pixel maps every index to 0
__device__ __forceinline__ int fold_index(long long i, int n, int mode) {
  if (n == 1) return 0;
  if (mode == GLARE_PAD_SYMMETRIC) {
    const long long per = 2LL * n;
    long long p = i % per;
    if (p < 0) p += per;
    return (int)(p < n ? p : per - 1 - p);
  }
  const long long per = 2LL * n - 2;
  long long p = i % per;
  if (p < 0) p += per;
  return (int)(p < n ? p : per - p);
}

// uint8 HWC [B][H][W][3] -> fp32 NCHW [B][3][Hp][Wp], one thread per output value (coalesced fp32 stores)
__global__ __launch_bounds__(256) void pre_pad_kernel(const uint8_t* __restrict__ img, int B, int H, int W, int top, int left, int Hp,
                                                      int Wp, int mode, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long plane = (long long)Hp * Wp;
  if (i >= (long long)B * 3 * plane) return;
  const long long bc = i / plane, r = i - bc * plane;
  const int y = (int)(r / Wp), x = (int)(r - (long long)y * Wp);
  const int b = (int)(bc / 3), c = (int)(bc - 3LL * b);
  const int ys = fold_index((long long)y - top, H, mode), xs = fold_index((long long)x - left, W, mode);
  const float v = (float)img[(((long long)b * H + ys) * W + xs) * 3 + c];
  out[i] = logf(fmaxf(__fdiv_rn(v, 255.f) + 1e-3f, 1e-3f));
}

constexpr int HBU = 128;  // blocks per image of the uint8 post-process (two int partials each: < glare_harness_postprocess_workspace_bytes)

// fp32 NCHW [B][3][Hp][Wp] -> uint8 HWC [B][h][w][3] of the window at (top, left): (uint8)(clamp(x, 0, 1) * 255), truncating
// (rgb(), infer_unpaired.py:42).  The output is one flat byte array; each thread writes one aligned 4-byte word of it.  A word
// belongs to the image of its first byte, so the last word of an image can carry the first bytes of the next one: their
// non-finite values go to a second partial (`spill`), and the per-image count stays a deterministic two-level integer sum.
__global__ __launch_bounds__(256) void post_u8_kernel(const float* __restrict__ out, int B, int Hp, int Wp, int top, int left, int h, int w,
                                                      uint8_t* __restrict__ dst, int* __restrict__ bad_partial) {
  __shared__ int red[2][4];
  const int b = blockIdx.y;
  const long long n = 3LL * h * w, total = n * B;
  const long long wlo = (n * b + 3) / 4, whi = (n * (b + 1) + 3) / 4;    // words whose first byte lies in image b
  int bad_own = 0, bad_next = 0;
  for (long long wd = wlo + (long long)blockIdx.x * 256 + threadIdx.x; wd < whi; wd += (long long)HBU * 256) {
    const long long k0 = wd * 4;
    int bk = b;
    long long r = k0 - n * b;
    const long long p = r / 3;
    int c = (int)(r - 3 * p);
    int y = (int)(p / w), x = (int)(p - (long long)y * w);
    uint32_t word = 0;
    const int nb = total - k0 < 4 ? (int)(total - k0) : 4;
    for (int j = 0; j < nb; ++j) {
      const float v = out[(((long long)bk * 3 + c) * Hp + top + y) * Wp + left + x];
      const int nf = (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;   // inf or NaN, counted BEFORE the clamp
      if (bk == b) bad_own += nf; else bad_next += nf;
      word |= (uint32_t)(uint8_t)(fminf(fmaxf(v, 0.f), 1.f) * 255.f) << (8 * j);
      if (++c == 3) { c = 0; if (++x == w) { x = 0; if (++y == h) { y = 0; ++bk; } } }
    }
    if (nb == 4) {
      *reinterpret_cast<uint32_t*>(dst + k0) = word;
    } else {
      for (int j = 0; j < nb; ++j) dst[k0 + j] = (uint8_t)(word >> (8 * j));
    }
  }
  if (!bad_partial) return;
  for (int o = 32; o > 0; o >>= 1) { bad_own += __shfl_xor(bad_own, o, 64); bad_next += __shfl_xor(bad_next, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = bad_own; red[1][threadIdx.x >> 6] = bad_next; }
  __syncthreads();
  if (threadIdx.x < 2)
    bad_partial[((size_t)threadIdx.x * B + b) * HBU + blockIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

__global__ void post_u8_count_kernel(const int* __restrict__ bad_partial, int B, int* __restrict__ nonfinite) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int s = 0;
  for (int k = 0; k < HBU; ++k) s += bad_partial[(size_t)b * HBU + k];                                  // own words
  if (b > 0)
    for (int k = 0; k < HBU; ++k) s += bad_partial[((size_t)B + b - 1) * HBU + k];                      // the previous image's last word
  nonfinite[b] = s;
}

// ---- the test scripts' "adjust" protocol (code/test_stage2.py:169-180, code/test_stage3.py:183-185, :203-204) ----------------
constexpr int HBS = 128;  // blocks per image of the two kernels below (glare_harness_score_workspace_bytes: two 8-byte partials each)

// level 1 of gain[b] = mean_gt / mean_out: per block, the fp64 sum of the window's RAW values (lr_out.reshape(B, -1).mean(1) is taken
// before any clamp, :169 / :183) and the sum of 114 g0 + 587 g1 + 299 g2 over the uint8 ground truth -- the COLOR_BGR2GRAY weights on
// RGB-ordered data (:170 / :184) in thousandths, which makes that half an exact integer.  One thread per pixel, grid-strided.
__global__ __launch_bounds__(256) void gain_partial_kernel(const float* __restrict__ out, const uint8_t* __restrict__ gt, int Hp, int Wp,
                                                           int top, int left, int h, int w, double* __restrict__ sum_out,
                                                           unsigned long long* __restrict__ sum_gt) {
  __shared__ double red[4];
  __shared__ unsigned long long redg[4];
  const int b = blockIdx.y;
  const long long npix = (long long)h * w;
  double sr = 0.0;
  unsigned long long sg = 0;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)HBS * 256) {
    const int y = (int)(p / w), x = (int)(p - (long long)y * w);
    const float* src = out + ((long long)b * 3 * Hp + top + y) * Wp + left + x;
    const long long plane = (long long)Hp * Wp;
    sr += ((double)src[0] + (double)src[plane]) + (double)src[2 * plane];
    const uint8_t* g = gt + ((long long)b * npix + p) * 3;
    sg += 114u * g[0] + 587u * g[1] + 299u * g[2];
  }
  for (int o = 32; o > 0; o >>= 1) { sr += __shfl_xor(sr, o, 64); sg += __shfl_xor(sg, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = sr; redg[threadIdx.x >> 6] = sg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    sum_out[(size_t)b * HBS + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    sum_gt[(size_t)b * HBS + blockIdx.x] = (redg[0] + redg[1]) + (redg[2] + redg[3]);
  }
}

// level 2: the HBS partials of an image in index order -> gain[b] = (float)(mean_gt / mean_out)
__global__ void gain_final_kernel(const double* __restrict__ sum_out, const unsigned long long* __restrict__ sum_gt, int B, long long npix,
                                  float* __restrict__ gain) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double sr = 0.0;
  unsigned long long sg = 0;
  for (int k = 0; k < HBS; ++k) { sr += sum_out[(size_t)b * HBS + k]; sg += sum_gt[(size_t)b * HBS + k]; }
  const double mean_out = sr / (3.0 * (double)npix);
  const double mean_gt = (double)sg / (1000.0 * 255.0 * (double)npix);
  gain[b] = (float)(mean_gt / mean_out);
}

// out_u8 = rgb(x * gain) = (uint8)(clamp(x * gain, 0, 1) * 255), truncating (rgb(), test_stage2.py:44-46; the clamp of :171 is the
// one rgb() repeats), and the integer sum of (out_u8 - gt_u8)^2 per image: what Measure.psnr (skimage's peak_signal_noise_ratio on
// two uint8 images) needs.  post_u8_kernel's layout: the output is one flat byte array, each thread owns one aligned 4-byte word of
// it and reads the ground truth's word at the same offset; a word belongs to the image of its first byte, so the squared error of
// the bytes it carries of the NEXT image goes to a second partial.  Integer partials: the sums are exact in any order.
__global__ __launch_bounds__(256) void score_u8_kernel(const float* __restrict__ out, const float* __restrict__ gain,
                                                       const uint8_t* __restrict__ gt, int B, int Hp, int Wp, int top, int left, int h, int w,
                                                       uint8_t* __restrict__ dst, unsigned long long* __restrict__ sse_partial) {
  __shared__ unsigned long long red[2][4];
  const int b = blockIdx.y;
  const long long n = 3LL * h * w, total = n * B;
  const long long wlo = (n * b + 3) / 4, whi = (n * (b + 1) + 3) / 4;    // words whose first byte lies in image b
  const float g_own = gain ? gain[b] : 1.f, g_next = gain && b + 1 < B ? gain[b + 1] : 1.f;
  unsigned long long sse_own = 0, sse_next = 0;
  for (long long wd = wlo + (long long)blockIdx.x * 256 + threadIdx.x; wd < whi; wd += (long long)HBS * 256) {
    const long long k0 = wd * 4;
    int bk = b;
    long long r = k0 - n * b;
    const long long p = r / 3;
    int c = (int)(r - 3 * p);
    int y = (int)(p / w), x = (int)(p - (long long)y * w);
    const int nb = total - k0 < 4 ? (int)(total - k0) : 4;
    uint32_t word = 0, gword = 0;
    if (nb == 4) {
      gword = *reinterpret_cast<const uint32_t*>(gt + k0);
    } else {
      for (int j = 0; j < nb; ++j) gword |= (uint32_t)gt[k0 + j] << (8 * j);
    }
    for (int j = 0; j < nb; ++j) {
      const float v = out[(((long long)bk * 3 + c) * Hp + top + y) * Wp + left + x] * (bk == b ? g_own : g_next);
      const uint32_t u = (uint8_t)(fminf(fmaxf(v, 0.f), 1.f) * 255.f);     // fmaxf(NaN, 0) = 0: a NaN (or 0 * inf) becomes 0
      const int d = (int)u - (int)((gword >> (8 * j)) & 0xffu);
      if (bk == b) sse_own += (unsigned)(d * d); else sse_next += (unsigned)(d * d);
      word |= u << (8 * j);
      if (++c == 3) { c = 0; if (++x == w) { x = 0; if (++y == h) { y = 0; ++bk; } } }
    }
    if (nb == 4) {
      *reinterpret_cast<uint32_t*>(dst + k0) = word;
    } else {
      for (int j = 0; j < nb; ++j) dst[k0 + j] = (uint8_t)(word >> (8 * j));
    }
  }
  for (int o = 32; o > 0; o >>= 1) { sse_own += __shfl_xor(sse_own, o, 64); sse_next += __shfl_xor(sse_next, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sse_own; red[1][threadIdx.x >> 6] = sse_next; }
  __syncthreads();
  if (threadIdx.x < 2)
    sse_partial[((size_t)threadIdx.x * B + b) * HBS + blockIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

__global__ void score_final_kernel(const unsigned long long* __restrict__ sse_partial, int B, long long* __restrict__ sse) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  unsigned long long s = 0;
  for (int k = 0; k < HBS; ++k) s += sse_partial[(size_t)b * HBS + k];                                  // own words
  if (b > 0)
    for (int k = 0; k < HBS; ++k) s += sse_partial[((size_t)B + b - 1) * HBS + k];                      // the previous image's last word
  sse[b] = (long long)s;
}

// ---- tiled enhancement (glare_amd.enhance.enhance_tiled): overlapping windows of one image, feathered back together ----------
// uint8 HWC [H][W][3] -> fp32 NCHW [n][3][th][tw]: window t starts at image coordinate (origins[2t], origins[2t + 1]), which may
// lie outside the image; such coordinates fold as pre_pad_kernel folds them, and the value is its expression, so a window that
// describes the pixels of a padded image carries that kernel's bits.  One thread per output value, 64-bit element offsets.
__global__ __launch_bounds__(256) void tile_gather_kernel(const uint8_t* __restrict__ img, int H, int W, const int* __restrict__ origins,
                                                          int n, int th, int tw, int mode, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long plane = (long long)th * tw;
  if (i >= (long long)n * 3 * plane) return;
  const long long tc = i / plane, r = i - tc * plane;
  const int y = (int)(r / tw), x = (int)(r - (long long)y * tw);
  const int t = (int)(tc / 3), c = (int)(tc - 3LL * t);
  const int ys = fold_index((long long)origins[2 * t] + y, H, mode), xs = fold_index((long long)origins[2 * t + 1] + x, W, mode);
  const float v = (float)img[((long long)ys * W + xs) * 3 + c];
  out[i] = logf(fmaxf(__fdiv_rn(v, 255.f) + 1e-3f, 1e-3f));
}

constexpr int HBT = 512;  // blocks of the blend (one int partial each: glare_harness_tile_blend_workspace_bytes)

// The network outputs of an image's n_ty x n_tx windows, fp32 NCHW [n_ty * n_tx][3][th][tw], window (i, j) at image coordinate
// (y0[i], x0[j]) -> the blended image: acc = sum_i sum_j fmaf(wy_i * wx_j, clamp(v_ij, 0, 1), acc), i and j ascending over the
// windows that cover the pixel, then (uint8)(fminf(acc, 1) * 255) as post_u8_kernel quantises.  Per axis and per coordinate the host
// supplies the first covering window, their number (<= 3) and their normalised weights (fc: int32 [L][2], wt: fp32 [L][3]), so the
// kernel divides nothing; a window the tables name but that does not hold the coordinate is skipped, never read.  post_u8_kernel's
// layout: the output is one flat byte array and each thread owns one aligned 4-byte word of it (and the 16 bytes of the optional
// fp32 image at the same element offset).  The count of raw inf / NaN values is an integer sum through one partial per block.
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ tiles, int n_ty, int n_tx, int th, int tw,
                                                         const int* __restrict__ y0, const int* __restrict__ x0, int H, int W,
                                                         const int* __restrict__ row_fc, const float* __restrict__ row_wt,
                                                         const int* __restrict__ col_fc, const float* __restrict__ col_wt,
                                                         uint8_t* __restrict__ dst, float* __restrict__ dst_f32,
                                                         int* __restrict__ bad_partial) {
  __shared__ int red[4];
  const long long total = 3LL * H * W, words = (total + 3) / 4;
  const long long plane = (long long)th * tw;
  int bad = 0;
  for (long long wd = (long long)blockIdx.x * 256 + threadIdx.x; wd < words; wd += (long long)HBT * 256) {
    const long long k0 = wd * 4;
    const long long p = k0 / 3;
    int c = (int)(k0 - 3 * p);
    int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const int nb = total - k0 < 4 ? (int)(total - k0) : 4;
    uint32_t word = 0;
    float a4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < nb) {
        const int fy = row_fc[2LL * y], ny = row_fc[2LL * y + 1], fx = col_fc[2LL * x], nx = col_fc[2LL * x + 1];
        float acc = 0.f;
        for (int a = 0; a < ny && a < 3; ++a) {
          const int ti = fy + a;
          if (ti < 0 || ti >= n_ty) continue;
          const int ly = y - y0[ti];
          if (ly < 0 || ly >= th) continue;
          const float wy = row_wt[3LL * y + a];
          for (int b = 0; b < nx && b < 3; ++b) {
            const int tj = fx + b;
            if (tj < 0 || tj >= n_tx) continue;
            const int lx = x - x0[tj];
            if (lx < 0 || lx >= tw) continue;
            const float v = tiles[(((long long)ti * n_tx + tj) * 3 + c) * plane + (long long)ly * tw + lx];
            bad += (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;   // inf or NaN, counted BEFORE the clamp, once per window
            acc = fmaf(wy * col_wt[3LL * x + b], fminf(fmaxf(v, 0.f), 1.f), acc);   // fmaxf(NaN, 0) = 0
          }
        }
        a4[j] = acc;
        word |= (uint32_t)(uint8_t)(fminf(acc, 1.f) * 255.f) << (8 * j);
        if (++c == 3) { c = 0; if (++x == W) { x = 0; ++y; } }
      }
    }
    if (nb == 4) {
      *reinterpret_cast<uint32_t*>(dst + k0) = word;
      if (dst_f32) *reinterpret_cast<float4*>(dst_f32 + k0) = make_float4(a4[0], a4[1], a4[2], a4[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j) {       // the last word of the image: 1 to 3 bytes
        if (j < nb) {
          dst[k0 + j] = (uint8_t)(word >> (8 * j));
          if (dst_f32) dst_f32[k0 + j] = a4[j];
        }
      }
    }
  }
  if (!bad_partial) return;
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0) bad_partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void tile_blend_count_kernel(const int* __restrict__ bad_partial, int* __restrict__ nonfinite) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int s = 0;
    for (int k = 0; k < HBT; ++k) s += bad_partial[k];
    *nonfinite = s;
  }
}

}  // namespace

// restored float in [0,1] -> uint8 = rint(clip * 255): img_as_ubyte(restored), the image the reference's loop hands to imwrite
__global__ __launch_bounds__(256) void to_ubyte_kernel(const float* __restrict__ restored, long long n, uint8_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (uint8_t)rintf(fminf(fmaxf(restored[i], 0.f), 1.f) * 255.f);
}

extern "C" int glare_harness_to_ubyte(const float* restored_hwc, long long n, unsigned char* out_u8, glare_stream_t stream) {
  if (!restored_hwc || !out_u8 || n <= 0) return GLARE_ERR_INVALID;
  hipLaunchKernelGGL(to_ubyte_kernel, dim3((unsigned)cdivll(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), restored_hwc, n, out_u8);
  return glare_launch_status();
}

extern "C" int glare_harness_ubyte_planes_f32(const float* restored_hwc, const unsigned char* gt_hwc, long long n, float* x255, float* y255,
                                              glare_stream_t stream) {
  if (!restored_hwc || !gt_hwc || !x255 || !y255 || n <= 0) return GLARE_ERR_INVALID;
  hipLaunchKernelGGL(ubyte_planes_kernel, dim3((unsigned)cdivll(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), restored_hwc,
                     gt_hwc, n, x255, y255);
  return glare_launch_status();
}

extern "C" int glare_harness_preprocess_u8(const unsigned char* img_hwc, int B, int H, int W, int pad, float* out_nchw,
                                           glare_stream_t stream) {
  if (!img_hwc || !out_nchw || B <= 0 || H <= 1 || W <= 1 || pad < 0) return GLARE_ERR_INVALID;
  const long long total = (long long)B * 3 * (H + pad) * (W + pad);
  hipLaunchKernelGGL(pre_kernel, dim3((unsigned)cdivll(total, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), img_hwc, B, H, W,
                     pad, out_nchw);
  return glare_launch_status();
}

extern "C" size_t glare_harness_postprocess_workspace_bytes(int B) { return B <= 0 ? 0 : (size_t)B * HB * (3 * sizeof(double) + sizeof(int)); }

extern "C" int glare_harness_postprocess_flagged_f32(const float* out_nchw, const unsigned char* gt_hwc_or_null, int B, int h, int w,
                                                     int Hp, int Wp, int pad, float* restored_hwc, double* psnr_or_null,
                                                     int* nonfinite_or_null, void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  if (!out_nchw || !restored_hwc || B <= 0 || h <= 0 || w <= 0 || h > Hp || w + pad > Wp || pad < 0) return GLARE_ERR_INVALID;
  if (psnr_or_null && !gt_hwc_or_null) return GLARE_ERR_INVALID;
  if (!workspace || workspace_bytes < glare_harness_postprocess_workspace_bytes(B)) return GLARE_ERR_WORKSPACE;
  double* partial = static_cast<double*>(workspace);
  double* mse_partial = partial + (size_t)B * HB * 2;
  int* bad_partial = reinterpret_cast<int*>(mse_partial + (size_t)B * HB);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(post_crop_kernel, dim3(HB, B), dim3(256), 0, s, out_nchw, gt_hwc_or_null, h, w, Hp, Wp, pad, restored_hwc, partial,
                     nonfinite_or_null ? bad_partial : (int*)nullptr);
  const long long n = (long long)h * w * 3;
  hipLaunchKernelGGL(post_gain_kernel, dim3(HB, B), dim3(256), 0, s, restored_hwc, gt_hwc_or_null, n, partial, gt_hwc_or_null ? 1 : 0,
                     mse_partial);
  if (psnr_or_null) hipLaunchKernelGGL(post_psnr_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, mse_partial, n, B, psnr_or_null);
  if (nonfinite_or_null) hipLaunchKernelGGL(post_count_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, bad_partial, B, nonfinite_or_null);
  return glare_launch_status();
}

extern "C" int glare_harness_postprocess_f32(const float* out_nchw, const unsigned char* gt_hwc_or_null, int B, int h, int w,
                                             int Hp, int Wp, int pad, float* restored_hwc, double* psnr_or_null, void* workspace,
                                             size_t workspace_bytes, glare_stream_t stream) {
  return glare_harness_postprocess_flagged_f32(out_nchw, gt_hwc_or_null, B, h, w, Hp, Wp, pad, restored_hwc, psnr_or_null, nullptr, workspace,
                                               workspace_bytes, stream);
}

extern "C" int glare_harness_preprocess_pad_u8(const unsigned char* img_hwc, int B, int H, int W, int top, int bottom, int left, int right,
                                               int mode, float* out_nchw, glare_stream_t stream) {
  if (!img_hwc || !out_nchw || B <= 0 || H <= 0 || W <= 0 || top < 0 || bottom < 0 || left < 0 || right < 0) return GLARE_ERR_INVALID;
  if (mode != GLARE_PAD_REFLECT101 && mode != GLARE_PAD_SYMMETRIC) return GLARE_ERR_INVALID;
  const long long Hp = (long long)H + top + bottom, Wp = (long long)W + left + right;
  if (Hp > 0x7fffffffLL || Wp > 0x7fffffffLL) return GLARE_ERR_INVALID;
  const long long blocks = cdivll((long long)B * 3 * Hp * Wp, 256);
  if (blocks > 0x7fffffffLL) return GLARE_ERR_INVALID;
  hipLaunchKernelGGL(pre_pad_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), img_hwc, B, H, W, top, left,
                     (int)Hp, (int)Wp, mode, out_nchw);
  return glare_launch_status();
}

extern "C" int glare_harness_postprocess_u8(const float* out_nchw, int B, int Hp, int Wp, int top, int left, int h, int w,
                                            unsigned char* out_hwc_u8, int* nonfinite_or_null, void* workspace, size_t workspace_bytes,
                                            glare_stream_t stream) {
  if (!out_nchw || !out_hwc_u8 || B <= 0 || h <= 0 || w <= 0 || top < 0 || left < 0) return GLARE_ERR_INVALID;
  if ((long long)top + h > Hp || (long long)left + w > Wp) return GLARE_ERR_INVALID;
  if (B > 65535 || 3LL * h * w > 0x7fffffffLL) return GLARE_ERR_INVALID;     // grid.y = B; one image's bytes, a word offset of 32 bits
  int* bad_partial = nullptr;
  if (nonfinite_or_null) {
    static_assert(HBU * 2 * sizeof(int) <= HB * (3 * sizeof(double) + sizeof(int)), "the partials fit the documented workspace");
    if (!workspace || workspace_bytes < glare_harness_postprocess_workspace_bytes(B)) return GLARE_ERR_WORKSPACE;
    bad_partial = static_cast<int*>(workspace);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(post_u8_kernel, dim3(HBU, B), dim3(256), 0, s, out_nchw, B, Hp, Wp, top, left, h, w, out_hwc_u8, bad_partial);
  if (nonfinite_or_null) hipLaunchKernelGGL(post_u8_count_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, bad_partial, B, nonfinite_or_null);
  return glare_launch_status();
}

// the window (top, left, h, w) of a [B][3][Hp][Wp] tensor as glare_harness_postprocess_u8 takes it: inside the tensor, grid.y = B,
// one image's bytes below 2^31
static bool score_window_ok(int B, int Hp, int Wp, int top, int left, int h, int w) {
  if (B <= 0 || B > 65535 || h <= 0 || w <= 0 || top < 0 || left < 0) return false;
  if ((long long)top + h > Hp || (long long)left + w > Wp) return false;
  return 3LL * h * w <= 0x7fffffffLL;
}

extern "C" size_t glare_harness_score_workspace_bytes(int B) { return B <= 0 ? 0 : (size_t)B * HBS * 2 * sizeof(unsigned long long); }

extern "C" int glare_harness_adjust_gain_f32(const float* out_nchw, const unsigned char* gt_hwc, int B, int Hp, int Wp, int top, int left,
                                             int h, int w, float* gain, void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  if (!out_nchw || !gt_hwc || !gain || !score_window_ok(B, Hp, Wp, top, left, h, w)) return GLARE_ERR_INVALID;
  if (!workspace || workspace_bytes < glare_harness_score_workspace_bytes(B)) return GLARE_ERR_WORKSPACE;
  static_assert(sizeof(double) == sizeof(unsigned long long), "the two partial arrays share one element size");
  double* sum_out = static_cast<double*>(workspace);
  unsigned long long* sum_gt = reinterpret_cast<unsigned long long*>(sum_out + (size_t)B * HBS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(gain_partial_kernel, dim3(HBS, B), dim3(256), 0, s, out_nchw, gt_hwc, Hp, Wp, top, left, h, w, sum_out, sum_gt);
  hipLaunchKernelGGL(gain_final_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, sum_out, sum_gt, B, (long long)h * w, gain);
  return glare_launch_status();
}

extern "C" int glare_harness_score_u8(const float* out_nchw, const float* gain_or_null, const unsigned char* gt_hwc, int B, int Hp, int Wp,
                                      int top, int left, int h, int w, unsigned char* out_hwc_u8, long long* sse, void* workspace,
                                      size_t workspace_bytes, glare_stream_t stream) {
  if (!out_nchw || !gt_hwc || !out_hwc_u8 || !sse || !score_window_ok(B, Hp, Wp, top, left, h, w)) return GLARE_ERR_INVALID;
  if (((uintptr_t)gt_hwc | (uintptr_t)out_hwc_u8) & 3) return GLARE_ERR_INVALID;      // both are read / written as 4-byte words
  if (!workspace || workspace_bytes < glare_harness_score_workspace_bytes(B)) return GLARE_ERR_WORKSPACE;
  unsigned long long* sse_partial = static_cast<unsigned long long*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(score_u8_kernel, dim3(HBS, B), dim3(256), 0, s, out_nchw, gain_or_null, gt_hwc, B, Hp, Wp, top, left, h, w, out_hwc_u8,
                     sse_partial);
  hipLaunchKernelGGL(score_final_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, sse_partial, B, sse);
  return glare_launch_status();
}

extern "C" int glare_harness_tile_gather_u8(const unsigned char* img_hwc, int H, int W, const int* origins_yx, int n, int th, int tw, int mode,
                                            float* out_nchw, glare_stream_t stream) {
  if (!img_hwc || !origins_yx || !out_nchw || H <= 0 || W <= 0 || n <= 0 || th <= 0 || tw <= 0) return GLARE_ERR_INVALID;
  if (mode != GLARE_PAD_REFLECT101 && mode != GLARE_PAD_SYMMETRIC) return GLARE_ERR_INVALID;
  if ((long long)th * tw > 0x7fffffffLL * 256 / 3 / n) return GLARE_ERR_INVALID;      // one thread per value, at most 2^31 - 1 blocks
  const long long blocks = cdivll((long long)n * 3 * th * tw, 256);
  hipLaunchKernelGGL(tile_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), img_hwc, H, W, origins_yx,
                     n, th, tw, mode, out_nchw);
  return glare_launch_status();
}

extern "C" size_t glare_harness_tile_blend_workspace_bytes(void) { return (size_t)HBT * sizeof(int); }

extern "C" int glare_harness_tile_blend_f32(const float* tiles_nchw, int n_ty, int n_tx, int th, int tw, const int* y0, const int* x0, int H,
                                            int W, const int* row_first_count, const float* row_weight, const int* col_first_count,
                                            const float* col_weight, unsigned char* out_hwc_u8, float* out_hwc_f32_or_null,
                                            int* nonfinite_or_null, void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  if (!tiles_nchw || !y0 || !x0 || !row_first_count || !row_weight || !col_first_count || !col_weight || !out_hwc_u8) return GLARE_ERR_INVALID;
  if (n_ty <= 0 || n_tx <= 0 || th <= 0 || tw <= 0 || H <= 0 || W <= 0) return GLARE_ERR_INVALID;
  if ((long long)n_ty * n_tx > 0x7fffffffLL) return GLARE_ERR_INVALID;
  if (((uintptr_t)out_hwc_u8 & 3) || ((uintptr_t)out_hwc_f32_or_null & 15)) return GLARE_ERR_INVALID;    // written as 4- and 16-byte words
  int* bad_partial = nullptr;
  if (nonfinite_or_null) {
    if (!workspace || workspace_bytes < glare_harness_tile_blend_workspace_bytes()) return GLARE_ERR_WORKSPACE;
    bad_partial = static_cast<int*>(workspace);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tile_blend_kernel, dim3(HBT), dim3(256), 0, s, tiles_nchw, n_ty, n_tx, th, tw, y0, x0, H, W, row_first_count, row_weight,
                     col_first_count, col_weight, out_hwc_u8, out_hwc_f32_or_null, bad_partial);
  if (nonfinite_or_null) hipLaunchKernelGGL(tile_blend_count_kernel, dim3(1), dim3(64), 0, s, bad_partial, nonfinite_or_null);
  return glare_launch_status();
}
