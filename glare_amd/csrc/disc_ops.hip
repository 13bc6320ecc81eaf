// The patch discriminator's layers around its 4x4 convs (conv4x4.hip), training form, and the hinge losses on its logits.
//
//   BatchNorm2d in training mode + LeakyReLU(0.2), NHWC 16-bit activations, fp32 statistics (nn.BatchNorm2d: eps 1e-5, affine, biased
//   variance for the normalisation, running_var from the unbiased one, momentum 0.1, num_batches_tracked):
//     mean[c] = sum x / n      var[c] = sum (x - mean)^2 / n      xhat = (x - mean) rstd,  rstd = 1 / sqrt(var + eps)
//     y = lrelu(gamma xhat + beta)
//     dz = dy lrelu'(gamma xhat + beta)   dbeta = sum dz   dgamma = sum dz xhat   dx = gamma rstd (dz - dbeta / n - xhat dgamma / n)
//   "batch groups": the batch is cut into `groups` runs of consecutive images and every statistic (forward and backward) is taken per
//   run, so the real and the fake batch pass through in ONE set of launches with the statistics two separate calls have; the running
//   statistics are then updated once per group in group order, exactly as two calls would, and dgamma / dbeta are the groups' sum.
//   The variance is the two-pass form (the mean first, then the squared deviations): a channel of constant input gives var ~ 0 without the
//   cancellation of E[x^2] - mean^2.
//
//   Hinge / generator losses on fp32 logits, with d loss / d x for a unit upstream gradient:
//     mode 0  mean relu(1 - x)   grad -[x < 1] / n        mode 1  mean relu(1 + x)   grad [x > -1] / n        mode 2  -mean x   grad -1 / n
//
// Every reduction has one order that depends on the shape alone: a thread walks a strided sub-sequence of its chunk in ascending order, the
// rows of a workgroup are added in row order, the chunks in chunk order, the groups in group order.  No atomics, no data-dependent address.
// Compiled with -ffp-contract=off: every rounding the bounds of tests/test_gpu_disc_kernels.py count is spelled here (fmaf where fused).
#include "common.h"

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_CHUNKS = 64;
constexpr int BN_CHUNK_MIN = 256;   // pixels per chunk at least
constexpr float LRELU_SLOPE = 0.2f;

struct BnGeo {
  long long n;       // pixels per group
  long long chunk;   // pixels per chunk
  int C, CT, R, S, G;
};

inline BnGeo bn_geo(int B, long long HW, int C, int groups) {
  BnGeo g;
  g.G = groups;
  g.C = C;
  g.n = (long long)(B / groups) * HW;
  int ct = 1;
  while (ct < C && ct < BN_THREADS) ct *= 2;
  g.CT = ct;
  g.R = BN_THREADS / ct;
  long long s = g.n / BN_CHUNK_MIN;
  g.S = (int)(s < 1 ? 1 : (s > BN_MAX_CHUNKS ? BN_MAX_CHUNKS : s));
  g.chunk = cdivll(g.n, g.S);
  return g;
}

// rows of a workgroup in row order: result valid in row 0
__device__ __forceinline__ float rows_sum_fixed(float v, float* red, int cl, int r, int CT, int R) {
  __syncthreads();
  red[r * CT + cl] = v;
  __syncthreads();
  if (r == 0)
    for (int k = 1; k < R; ++k) v = __fadd_rn(v, red[k * CT + cl]);
  return v;
}

__device__ __forceinline__ float chunks_sum(const float* part, int S, long long stride) {
  float m = part[0];
  for (int s = 1; s < S; ++s) m = __fadd_rn(m, part[(long long)s * stride]);
  return m;
}

// MODE 0: part[g][s][c] = sum x;   MODE 1: sum (x - mean)^2, mean from MODE 0's partials
template <int MODE>
__global__ __launch_bounds__(BN_THREADS) void bn_stat_kernel(const a16_t* __restrict__ x, const BnGeo q, const float* __restrict__ sum_part,
                                                              float* __restrict__ part) {
  __shared__ float red[BN_THREADS];
  const int cl = threadIdx.x % q.CT, r = threadIdx.x / q.CT;
  const int c = blockIdx.y * q.CT + cl, g = blockIdx.z, s = blockIdx.x;
  const long long p0 = (long long)s * q.chunk, p1 = p0 + q.chunk < q.n ? p0 + q.chunk : q.n;
  float acc = 0.f, mean = 0.f;
  if (c < q.C) {
    if (MODE == 1) mean = chunks_sum(sum_part + (long long)g * q.S * q.C + c, q.S, q.C) / (float)q.n;
    const a16_t* xg = x + (long long)g * q.n * q.C + c;
    for (long long pix = p0 + r; pix < p1; pix += q.R) {
      const float v = a2f(xg[pix * q.C]);
      if (MODE == 0) {
        acc = __fadd_rn(acc, v);
      } else {
        const float d = __fsub_rn(v, mean);
        acc = __fadd_rn(acc, __fmul_rn(d, d));
      }
    }
  }
  acc = rows_sum_fixed(acc, red, cl, r, q.CT, q.R);
  if (r == 0 && c < q.C) part[((long long)g * q.S + s) * q.C + c] = acc;
}

// thread = one channel, the groups in order: saved[g][0][c] = mean, saved[g][1][c] = rstd; the running statistics once per group
__global__ __launch_bounds__(BN_THREADS) void bn_finalize_kernel(const BnGeo q, const float* __restrict__ sum_part, const float* __restrict__ sq_part,
                                                                  float eps, float momentum, float* __restrict__ saved, float* __restrict__ running_mean,
                                                                  float* __restrict__ running_var, long long* __restrict__ num_batches_tracked) {
  const int c = blockIdx.x * BN_THREADS + threadIdx.x;
  if (c == 0 && num_batches_tracked) *num_batches_tracked += q.G;
  if (c >= q.C) return;
  const float nf = (float)q.n;
  for (int g = 0; g < q.G; ++g) {
    const float mean = chunks_sum(sum_part + (long long)g * q.S * q.C + c, q.S, q.C) / nf;
    const float var = chunks_sum(sq_part + (long long)g * q.S * q.C + c, q.S, q.C) / nf;
    saved[((long long)g * 2 + 0) * q.C + c] = mean;
    saved[((long long)g * 2 + 1) * q.C + c] = 1.0f / sqrtf(__fadd_rn(var, eps));
    if (running_mean) running_mean[c] = __fadd_rn(__fmul_rn(1.0f - momentum, running_mean[c]), __fmul_rn(momentum, mean));
    if (running_var) {
      const float unbiased = q.n > 1 ? __fmul_rn(var, nf / (float)(q.n - 1)) : var;
      running_var[c] = __fadd_rn(__fmul_rn(1.0f - momentum, running_var[c]), __fmul_rn(momentum, unbiased));
    }
  }
}

__device__ __forceinline__ float lrelu_(float z, int on) { return (on && !(z > 0.f)) ? __fmul_rn(LRELU_SLOPE, z) : z; }

__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const a16_t* __restrict__ x, a16_t* __restrict__ y, const BnGeo q, const float* __restrict__ saved,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, int lrelu, long long total) {
  const long long i = (long long)blockIdx.x * BN_THREADS + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % q.C);
  const int g = (int)((i / q.C) / q.n);
  const float mean = saved[((long long)g * 2 + 0) * q.C + c], rstd = saved[((long long)g * 2 + 1) * q.C + c];
  const float xhat = __fmul_rn(__fsub_rn(a2f(x[i]), mean), rstd);
  y[i] = f2a(lrelu_(fmaf(xhat, gamma[c], beta[c]), lrelu));
}

// part[g][s][0][c] = sum dz, part[g][s][1][c] = sum dz xhat
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_stat_kernel(const a16_t* __restrict__ x, const a16_t* __restrict__ dy, const BnGeo q,
                                                                  const float* __restrict__ saved, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, int lrelu, float* __restrict__ part) {
  __shared__ float red[BN_THREADS];
  const int cl = threadIdx.x % q.CT, r = threadIdx.x / q.CT;
  const int c = blockIdx.y * q.CT + cl, g = blockIdx.z, s = blockIdx.x;
  const long long p0 = (long long)s * q.chunk, p1 = p0 + q.chunk < q.n ? p0 + q.chunk : q.n;
  float a0 = 0.f, a1 = 0.f;
  if (c < q.C) {
    const float mean = saved[((long long)g * 2 + 0) * q.C + c], rstd = saved[((long long)g * 2 + 1) * q.C + c];
    const float ga = gamma[c], be = beta[c];
    const long long base = (long long)g * q.n * q.C + c;
    for (long long pix = p0 + r; pix < p1; pix += q.R) {
      const float xhat = __fmul_rn(__fsub_rn(a2f(x[base + pix * q.C]), mean), rstd);
      const float z = fmaf(xhat, ga, be);
      float d = a2f(dy[base + pix * q.C]);
      if (lrelu && !(z > 0.f)) d = __fmul_rn(LRELU_SLOPE, d);
      a0 = __fadd_rn(a0, d);
      a1 = fmaf(d, xhat, a1);
    }
  }
  a0 = rows_sum_fixed(a0, red, cl, r, q.CT, q.R);
  a1 = rows_sum_fixed(a1, red, cl, r, q.CT, q.R);
  if (r == 0 && c < q.C) {
    part[(((long long)g * q.S + s) * 2 + 0) * q.C + c] = a0;
    part[(((long long)g * q.S + s) * 2 + 1) * q.C + c] = a1;
  }
}

// thread = one channel: gsum[g][0|1][c] = the group's two sums (chunk order); dbeta / dgamma = their sum in group order
__global__ __launch_bounds__(BN_THREADS) void bn_bwd_finalize_kernel(const BnGeo q, const float* __restrict__ part, float* __restrict__ gsum,
                                                                      float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * BN_THREADS + threadIdx.x;
  if (c >= q.C) return;
  float tb = 0.f, tg = 0.f;
  for (int g = 0; g < q.G; ++g) {
    const float sb = chunks_sum(part + ((long long)g * q.S * 2 + 0) * q.C + c, q.S, 2ll * q.C);
    const float sg = chunks_sum(part + ((long long)g * q.S * 2 + 1) * q.C + c, q.S, 2ll * q.C);
    gsum[((long long)g * 2 + 0) * q.C + c] = sb;
    gsum[((long long)g * 2 + 1) * q.C + c] = sg;
    tb = g == 0 ? sb : __fadd_rn(tb, sb);
    tg = g == 0 ? sg : __fadd_rn(tg, sg);
  }
  dbeta[c] = tb;
  dgamma[c] = tg;
}

__global__ __launch_bounds__(BN_THREADS) void bn_bwd_apply_kernel(const a16_t* __restrict__ x, const a16_t* __restrict__ dy, a16_t* __restrict__ dx, const BnGeo q,
                                                                   const float* __restrict__ saved, const float* __restrict__ gsum,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta, int lrelu,
                                                                   long long total) {
  const long long i = (long long)blockIdx.x * BN_THREADS + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % q.C);
  const int g = (int)((i / q.C) / q.n);
  const float mean = saved[((long long)g * 2 + 0) * q.C + c], rstd = saved[((long long)g * 2 + 1) * q.C + c];
  const float nf = (float)q.n;
  const float mb = gsum[((long long)g * 2 + 0) * q.C + c] / nf, mg = gsum[((long long)g * 2 + 1) * q.C + c] / nf;
  const float xhat = __fmul_rn(__fsub_rn(a2f(x[i]), mean), rstd);
  const float z = fmaf(xhat, gamma[c], beta[c]);
  float d = a2f(dy[i]);
  if (lrelu && !(z > 0.f)) d = __fmul_rn(LRELU_SLOPE, d);
  const float t = __fsub_rn(__fsub_rn(d, mb), __fmul_rn(xhat, mg));
  dx[i] = f2a(__fmul_rn(__fmul_rn(gamma[c], rstd), t));
}

// LeakyReLU(0.2) fused behind a conv (layer 1, no norm): g *= (y > 0 ? 1 : 0.2), y the conv's stored output (same sign as its input)
__global__ __launch_bounds__(BN_THREADS) void lrelu_bwd_kernel(const a16_t* __restrict__ g, const a16_t* __restrict__ y, a16_t* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * BN_THREADS + threadIdx.x;
  if (i >= n) return;
  const float d = a2f(g[i]);
  out[i] = (a2f(y[i]) > 0.f) ? g[i] : f2a(__fmul_rn(LRELU_SLOPE, d));
}

// ---- hinge -------------------------------------------------------------------------------------------------------------------------
constexpr int HG_THREADS = 256;
constexpr int HG_MAX_SPANS = 1024;
constexpr int HG_SPAN_MIN = 2048;

__device__ __forceinline__ float block_sum_fixed(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = HG_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = __fadd_rn(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(HG_THREADS) void hinge_span_kernel(const float* __restrict__ x, long long n, long long span, int mode, float inv_n,
                                                                 float* __restrict__ grad, float* __restrict__ partial) {
  __shared__ float red[HG_THREADS];
  const long long e0 = (long long)blockIdx.x * span;
  const long long e1 = e0 + span < n ? e0 + span : n;
  float acc = 0.f;
  for (long long e = e0 + threadIdx.x; e < e1; e += HG_THREADS) {
    const float v = x[e];
    // selects, not a branch per mode (the three-way uniform branch lost the mode-2 value of t in the compiler's lowering)
    const float u = mode == 0 ? __fsub_rn(1.0f, v) : __fadd_rn(1.0f, v);
    const bool on = u > 0.f;
    const float t = mode == 2 ? -v : (on ? u : 0.f);
    const float g = mode == 2 ? -inv_n : (on ? (mode == 0 ? -inv_n : inv_n) : 0.f);
    acc = __fadd_rn(acc, t);
    if (grad) grad[e] = g;
  }
  const float s = block_sum_fixed(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(HG_THREADS) void hinge_final_kernel(const float* __restrict__ partial, int n_spans, float nf, float* __restrict__ out) {
  __shared__ float red[HG_THREADS];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_spans; i += HG_THREADS) acc = __fadd_rn(acc, partial[i]);
  const float s = block_sum_fixed(acc, red);
  if (threadIdx.x == 0) out[0] = s / nf;
}

inline int hinge_spans(long long n) {
  const long long s = cdivll(n, HG_SPAN_MIN);
  return (int)(s < 1 ? 1 : (s > HG_MAX_SPANS ? HG_MAX_SPANS : s));
}

inline int bn_check(int B, long long HW, int C, int groups) {
  if (B <= 0 || HW <= 0 || C <= 0 || groups <= 0 || B % groups != 0) return GLARE_ERR_INVALID;
  if (groups > 65535 || cdiv(C, BN_THREADS) > 65535) return GLARE_ERR_UNSUPPORTED;
  if ((double)B * (double)HW * (double)C >= 9.0e18) return GLARE_ERR_UNSUPPORTED;
  if (cdivll((long long)B * HW * C, BN_THREADS) > 0x7fffffffLL) return GLARE_ERR_UNSUPPORTED;   // one thread per element in the apply kernels
  return GLARE_OK;
}

}  // namespace

#define ST(s) static_cast<hipStream_t>(s)

extern "C" size_t glare_batchnorm_workspace_bytes(int B, long long HW, int C, int groups) {
  if (bn_check(B, HW, C, groups) != GLARE_OK) return 0;
  const BnGeo q = bn_geo(B, HW, C, groups);
  // forward: two partial blocks [G][S][C]; backward: [G][S][2][C] + [G][2][C]
  return ((size_t)q.G * q.S * 2 * C + (size_t)q.G * 2 * C) * sizeof(float);
}

extern "C" int glare_batchnorm_lrelu_bf16(const void* x, const float* gamma, const float* beta, void* y, int B, long long HW, int C, int groups,
                                          float eps, float momentum, int lrelu, float* saved_stats, float* running_mean, float* running_var,
                                          long long* num_batches_tracked, void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  const int rc = bn_check(B, HW, C, groups);
  if (rc != GLARE_OK) return rc;
  if (!x || !gamma || !beta || !y || !saved_stats || !workspace) return GLARE_ERR_INVALID;
  if (workspace_bytes < glare_batchnorm_workspace_bytes(B, HW, C, groups)) return GLARE_ERR_WORKSPACE;
  const BnGeo q = bn_geo(B, HW, C, groups);
  float* sum_part = static_cast<float*>(workspace);
  float* sq_part = sum_part + (size_t)q.G * q.S * C;
  const dim3 sgrid((unsigned)q.S, (unsigned)cdiv(C, q.CT), (unsigned)q.G);
  const long long total = (long long)B * HW * C;
  hipLaunchKernelGGL(bn_stat_kernel<0>, sgrid, dim3(BN_THREADS), 0, ST(stream), static_cast<const a16_t*>(x), q, nullptr, sum_part);
  hipLaunchKernelGGL(bn_stat_kernel<1>, sgrid, dim3(BN_THREADS), 0, ST(stream), static_cast<const a16_t*>(x), q, sum_part, sq_part);
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)cdiv(C, BN_THREADS)), dim3(BN_THREADS), 0, ST(stream), q, sum_part, sq_part, eps, momentum,
                     saved_stats, running_mean, running_var, num_batches_tracked);
  hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)cdivll(total, BN_THREADS)), dim3(BN_THREADS), 0, ST(stream), static_cast<const a16_t*>(x),
                     static_cast<a16_t*>(y), q, saved_stats, gamma, beta, lrelu ? 1 : 0, total);
  return glare_launch_status();
}

extern "C" int glare_batchnorm_lrelu_backward_bf16(const void* x, const void* dy, const float* saved_stats, const float* gamma, const float* beta,
                                                   void* dx, float* dgamma, float* dbeta, int B, long long HW, int C, int groups, int lrelu,
                                                   void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  const int rc = bn_check(B, HW, C, groups);
  if (rc != GLARE_OK) return rc;
  if (!x || !dy || !saved_stats || !gamma || !beta || !dx || !dgamma || !dbeta || !workspace) return GLARE_ERR_INVALID;
  if (workspace_bytes < glare_batchnorm_workspace_bytes(B, HW, C, groups)) return GLARE_ERR_WORKSPACE;
  const BnGeo q = bn_geo(B, HW, C, groups);
  float* part = static_cast<float*>(workspace);
  float* gsum = part + (size_t)q.G * q.S * 2 * C;
  const dim3 sgrid((unsigned)q.S, (unsigned)cdiv(C, q.CT), (unsigned)q.G);
  const long long total = (long long)B * HW * C;
  hipLaunchKernelGGL(bn_bwd_stat_kernel, sgrid, dim3(BN_THREADS), 0, ST(stream), static_cast<const a16_t*>(x), static_cast<const a16_t*>(dy), q,
                     saved_stats, gamma, beta, lrelu ? 1 : 0, part);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)cdiv(C, BN_THREADS)), dim3(BN_THREADS), 0, ST(stream), q, part, gsum, dgamma, dbeta);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)cdivll(total, BN_THREADS)), dim3(BN_THREADS), 0, ST(stream), static_cast<const a16_t*>(x),
                     static_cast<const a16_t*>(dy), static_cast<a16_t*>(dx), q, saved_stats, gsum, gamma, beta, lrelu ? 1 : 0, total);
  return glare_launch_status();
}

extern "C" int glare_lrelu_backward_bf16(const void* g, const void* y, void* out, long long n, glare_stream_t stream) {
  if (n < 0) return GLARE_ERR_INVALID;
  if (n == 0) return GLARE_OK;
  if (!g || !y || !out) return GLARE_ERR_INVALID;
  if (cdivll(n, BN_THREADS) > 0x7fffffffLL) return GLARE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(lrelu_bwd_kernel, dim3((unsigned)cdivll(n, BN_THREADS)), dim3(BN_THREADS), 0, ST(stream), static_cast<const a16_t*>(g),
                     static_cast<const a16_t*>(y), static_cast<a16_t*>(out), n);
  return glare_launch_status();
}

extern "C" size_t glare_hinge_workspace_bytes(long long n) { return n <= 0 ? 0 : (size_t)hinge_spans(n) * sizeof(float); }

extern "C" int glare_hinge_loss_f32(const float* x, long long n, int mode, float* loss, float* grad, void* workspace, size_t workspace_bytes,
                                    glare_stream_t stream) {
  if (n <= 0 || mode < 0 || mode > 2) return GLARE_ERR_INVALID;
  if (!x || !loss || !workspace) return GLARE_ERR_INVALID;
  if (n >= (1ll << 24)) return GLARE_ERR_UNSUPPORTED;     // (float)n is exact below 2^24: the mean's divisor is n itself
  const int spans = hinge_spans(n);
  if (workspace_bytes < (size_t)spans * sizeof(float)) return GLARE_ERR_WORKSPACE;
  const long long span = cdivll(n, spans);
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(hinge_span_kernel, dim3((unsigned)spans), dim3(HG_THREADS), 0, ST(stream), x, n, span, mode, 1.0f / (float)n, grad, partial);
  hipLaunchKernelGGL(hinge_final_kernel, dim3(1), dim3(HG_THREADS), 0, ST(stream), partial, spans, (float)n, loss);
  return glare_launch_status();
}
