// Codebook layer, EMA form: the per-code statistics of a step's tokens and the exponential-moving-average update of the codebook.
//
// Replaces EmbeddingEMA.{cluster_size_ema_update, embed_avg_ema_update, weight_update} and the one-hot statistics EMAVectorQuantizer.forward
// feeds them (reference: code/models/modules/quantize.py:345-358, 426-434).  Semantics: include/glare_hip.h.
//   glare_vq_ema_stats_f32    idx [N], z [N][3] -> stats [K][4] = {s_k0, s_k1, s_k2, n_k}: n_k the tokens that select code k, s_k their sum
//   glare_vq_ema_update_f32   cluster_size = d cluster_size + (1 - d) n_k;  embed_avg = d embed_avg + (1 - d) s_k;  n = sum_k cluster_size;
//                             E_k = embed_avg_k / ((cluster_size_k + eps) / (n + K eps) * n);  n == 0: E is left as it was
// Two entries, so that `stats` can be summed over ranks in between.
//
// Everything is bitwise reproducible: no atomics of any kind, every sum has one order that depends on (N, K) alone.
//   stats   the walk of vq_de_segment_kernel (vq_train.hip) over another quantity: the token axis is cut into S <= 32 equal segments, a
//           workgroup stages 512 tokens {z0, z1, z2, index} at a time in LDS, thread (code k, segment s) reads them back as wave-uniform
//           broadcasts in token order and adds z of the tokens whose index is k; the count is an INTEGER.  S == 1 writes stats itself
//           (one launch); otherwise a second launch adds the S partial rows of a code in segment order.  The count becomes a float at the
//           very end: exact, as N <= 2^24 is asked.  No store address depends on a loaded index: an index outside [0, K) selects nothing
//           and cannot fault.
//   update  launch 1: thread = code, both EMAs, and the workgroup's sum of the NEW cluster sizes: a fixed LDS tree IN FP64
//           launch 2: ONE workgroup adds the <= 4096 workgroup sums, each thread its strided sub-sequence in ascending order, then the
//                     same fixed tree, still in fp64: n
//           launch 3: thread = code: the row.
//           n is HELD IN FP64 through both levels (the sum of K <= 2^20 fp32 values in fp64 is off by < K 2^-53 relative: nothing next to
//           one fp32 rounding) and rounded to fp32 ONCE, in launch 3; every operation after that is fp32.  The error bounds of
//           tests/test_gpu_vq_ema.py count that one rounding.  1 - d is formed in fp32 (exact for d >= 0.5).
// Compiled with -ffp-contract=off like the other vq*.hip: every rounding the bounds count is spelled here.
#include "common.h"

namespace {

constexpr int VE_THREADS = 256;
constexpr int VE_MAX_SEGMENTS = 32;    // token segments of the per-code sum (vq_train.hip's rule)
constexpr int VE_SEGMENT_MIN = 512;    // tokens per segment at least
constexpr int VE_TILE = 512;           // tokens of a segment resident in LDS at once (x 16 B = 8 KB)
constexpr long long VE_MAX_TOKENS = 1ll << 24;     // the float count stays exact

int n_segments(long long n_tokens) {
  const long long s = cdivll(n_tokens, VE_SEGMENT_MIN);
  return (int)(s < 1 ? 1 : (s > VE_MAX_SEGMENTS ? VE_MAX_SEGMENTS : s));
}

// thread = one code, blockIdx.y = one token segment -> out[seg][code][4] = {sum z0, sum z1, sum z2, count}; the count is written as a
// float when this is the only segment (out = stats), as its integer bits otherwise (out = the partial rows)
__global__ __launch_bounds__(VE_THREADS) void vq_ema_segment_kernel(const long long* __restrict__ idx, const float* __restrict__ z,
                                                                     long long n_tokens, int n_codes, long long seg_len, int single,
                                                                     float* __restrict__ out) {
  __shared__ f32x4 tile[VE_TILE];
  const int code = blockIdx.x * VE_THREADS + threadIdx.x;
  const long long t0 = (long long)blockIdx.y * seg_len;
  const long long t1 = t0 + seg_len < n_tokens ? t0 + seg_len : n_tokens;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  int cnt = 0;
  for (long long base = t0; base < t1; base += VE_TILE) {
    const int nt = (int)(t1 - base < VE_TILE ? t1 - base : VE_TILE);
    __syncthreads();
    for (int t = threadIdx.x; t < nt; t += VE_THREADS) {
      const long long tok = base + t;
      const long long k = idx[tok];
      f32x4 v;
      v[0] = z[tok * 3 + 0];
      v[1] = z[tok * 3 + 1];
      v[2] = z[tok * 3 + 2];
      v[3] = __int_as_float((k >= 0 && k < (long long)n_codes) ? (int)k : -1);    // an index out of range selects no code
      tile[t] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < nt; ++t) {
      const f32x4 v = tile[t];               // wave-uniform address: one broadcast ds_read_b128
      if (__float_as_int(v[3]) == code) {
        a0 = __fadd_rn(a0, v[0]);
        a1 = __fadd_rn(a1, v[1]);
        a2 = __fadd_rn(a2, v[2]);
        ++cnt;
      }
    }
  }
  if (code < n_codes) {
    float* p = out + ((long long)blockIdx.y * n_codes + code) * 4;
    p[0] = a0;
    p[1] = a1;
    p[2] = a2;
    p[3] = single ? (float)cnt : __int_as_float(cnt);
  }
}

// thread = one code: the segments' partial rows in segment order
__global__ __launch_bounds__(VE_THREADS) void vq_ema_final_kernel(const float* __restrict__ partial, int segs, int n_codes,
                                                                   float* __restrict__ stats) {
  const int code = blockIdx.x * VE_THREADS + threadIdx.x;
  if (code >= n_codes) return;
  const float* p = partial + (long long)code * 4;
  float a0 = p[0], a1 = p[1], a2 = p[2];
  int cnt = __float_as_int(p[3]);
  for (int s = 1; s < segs; ++s) {
    p = partial + ((long long)s * n_codes + code) * 4;
    a0 = __fadd_rn(a0, p[0]);
    a1 = __fadd_rn(a1, p[1]);
    a2 = __fadd_rn(a2, p[2]);
    cnt += __float_as_int(p[3]);
  }
  float* o = stats + (long long)code * 4;
  o[0] = a0;
  o[1] = a1;
  o[2] = a2;
  o[3] = (float)cnt;                         // <= 2^24: exact
}

// fixed-order fp64 sum of one value per thread over a 256-thread workgroup: result valid in thread 0
__device__ __forceinline__ double block_sum_fixed_f64(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = VE_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(VE_THREADS) void vq_ema_state_kernel(const float* __restrict__ stats, int K, float decay,
                                                                   float* __restrict__ cluster_size, float* __restrict__ embed_avg,
                                                                   double* __restrict__ group_sum) {
  __shared__ double red[VE_THREADS];
  const int k = blockIdx.x * VE_THREADS + threadIdx.x;
  const float alpha = __fsub_rn(1.f, decay);
  float cs = 0.f;
  if (k < K) {
    const float* st = stats + (size_t)k * 4;
    cs = __fadd_rn(__fmul_rn(cluster_size[k], decay), __fmul_rn(alpha, st[3]));          // quantize.py:346
    cluster_size[k] = cs;
    float* ea = embed_avg + (size_t)k * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) ea[c] = __fadd_rn(__fmul_rn(ea[c], decay), __fmul_rn(alpha, st[c]));      // :349
  }
  const double s = block_sum_fixed_f64((double)cs, red);
  if (threadIdx.x == 0) group_sum[blockIdx.x] = s;
}

__global__ __launch_bounds__(VE_THREADS) void vq_ema_total_kernel(const double* __restrict__ group_sum, int groups, double* __restrict__ n_out) {
  __shared__ double red[VE_THREADS];
  double acc = 0.0;
  for (int g = threadIdx.x; g < groups; g += VE_THREADS) acc = acc + group_sum[g];
  const double s = block_sum_fixed_f64(acc, red);
  if (threadIdx.x == 0) n_out[0] = s;
}

__global__ __launch_bounds__(VE_THREADS) void vq_ema_rows_kernel(const float* __restrict__ cluster_size, const float* __restrict__ embed_avg,
                                                                  const double* __restrict__ n_in, int K, float eps,
                                                                  float* __restrict__ codebook) {
  const int k = blockIdx.x * VE_THREADS + threadIdx.x;
  if (k >= K) return;
  const double n64 = n_in[0];
  if (n64 == 0.0) return;                    // the reference would write 0 / 0 (quantize.py:354): the rows stay as they were
  const float n = __double2float_rn(n64);    // the one rounding of n
  const float den = __fadd_rn(n, __fmul_rn((float)K, eps));
  const float smoothed = __fmul_rn(__fdiv_rn(__fadd_rn(cluster_size[k], eps), den), n);              // :353-355
  const float* ea = embed_avg + (size_t)k * 3;
  float* row = codebook + (size_t)k * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) row[c] = __fdiv_rn(ea[c], smoothed);                                    // :357-358
}

size_t update_bytes(int n_codes) { return ((size_t)cdiv(n_codes, VE_THREADS) + 1) * sizeof(double); }

}  // namespace

extern "C" size_t glare_vq_ema_workspace_bytes(long long n_tokens, int n_codes) {
  if (n_tokens <= 0 || n_tokens > VE_MAX_TOKENS || n_codes <= 0 || n_codes > GLARE_VQ_USAGE_MAX_CODES) return 0;
  const int segs = n_segments(n_tokens);
  const size_t stats = segs > 1 ? (size_t)segs * (size_t)n_codes * 4 * sizeof(float) : 0;      // the partial rows
  const size_t update = update_bytes(n_codes);                                                  // the workgroup sums, then n
  return stats > update ? stats : update;
}

extern "C" int glare_vq_ema_stats_f32(const long long* idx_i64, const float* z_tokens, long long n_tokens, int n_codes, int dim, float* stats,
                                      void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  if (n_tokens <= 0 || n_codes <= 0 || dim <= 0) return GLARE_ERR_INVALID;
  if (!idx_i64 || !z_tokens || !stats || !workspace) return GLARE_ERR_INVALID;
  if (((uintptr_t)workspace & 7u) != 0) return GLARE_ERR_INVALID;
  if (dim != 3 || n_tokens > VE_MAX_TOKENS || n_codes > GLARE_VQ_USAGE_MAX_CODES) return GLARE_ERR_UNSUPPORTED;
  if (workspace_bytes < glare_vq_ema_workspace_bytes(n_tokens, n_codes)) return GLARE_ERR_WORKSPACE;
  const int segs = n_segments(n_tokens);
  const long long seg_len = cdivll(n_tokens, segs);
  const unsigned groups = (unsigned)cdiv(n_codes, VE_THREADS);
  float* partial = reinterpret_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(vq_ema_segment_kernel, dim3(groups, (unsigned)segs), dim3(VE_THREADS), 0, s, idx_i64, z_tokens, n_tokens, n_codes, seg_len,
                     segs == 1 ? 1 : 0, segs == 1 ? stats : partial);
  if (segs > 1) hipLaunchKernelGGL(vq_ema_final_kernel, dim3(groups), dim3(VE_THREADS), 0, s, partial, segs, n_codes, stats);
  return glare_launch_status();
}

extern "C" int glare_vq_ema_update_f32(const float* stats, int n_codes, int dim, float decay, float eps, float* cluster_size, float* embed_avg,
                                       float* codebook, void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  if (n_codes <= 0 || dim <= 0) return GLARE_ERR_INVALID;
  if (!stats || !cluster_size || !embed_avg || !codebook || !workspace) return GLARE_ERR_INVALID;
  if (!(decay > 0.f && decay < 1.f) || !(eps >= 0.f)) return GLARE_ERR_INVALID;
  if (((uintptr_t)workspace & 7u) != 0) return GLARE_ERR_INVALID;
  if (dim != 3 || n_codes > GLARE_VQ_USAGE_MAX_CODES) return GLARE_ERR_UNSUPPORTED;
  if (workspace_bytes < update_bytes(n_codes)) return GLARE_ERR_WORKSPACE;
  const int groups = cdiv(n_codes, VE_THREADS);
  double* group_sum = reinterpret_cast<double*>(workspace);
  double* n = group_sum + groups;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(vq_ema_state_kernel, dim3((unsigned)groups), dim3(VE_THREADS), 0, s, stats, n_codes, decay, cluster_size, embed_avg,
                     group_sum);
  hipLaunchKernelGGL(vq_ema_total_kernel, dim3(1), dim3(VE_THREADS), 0, s, group_sum, groups, n);
  hipLaunchKernelGGL(vq_ema_rows_kernel, dim3((unsigned)groups), dim3(VE_THREADS), 0, s, cluster_size, embed_avg, n, n_codes, eps, codebook);
  return glare_launch_status();
}
