// Codebook layer, training form: the loss sum, the straight-through output and the gradients of the latent and of the codebook.
//
// Replaces the loss and the straight-through estimator of VectorQuantizer2.forward (reference: code/models/modules/quantize.py:289-298)
// and what autograd derives from them:
//   loss = (w_z + w_e) * S / (3 N),  S = sum_i sum_c (z_q[i,c] - z[i,c])^2        (w_z, w_e) = (beta, 1), legacy: (1, beta)
//   z_st = z + (z_q - z)
//   dz[i] = g[i] + gl * (2 w_z / 3N) * (z[i] - z_q[i])
//   dE[k] = gl * (2 w_e / 3N) * sum_{i : idx[i] = k} (z_q[i] - z[i])              a code no token selected: exactly 0
// The indices and z_q come from glare_vq_nearest_f32 (vq.hip), which this file does not touch.
//
// Everything here is bitwise reproducible: no atomics of any kind, every sum has one order that depends on (N, K) alone.
//   S   two levels: a workgroup sums a contiguous span of the 3N elements (each lane a strided sub-sequence in ascending order, then a
//       fixed LDS tree), one workgroup sums the <= 1024 span sums the same way.
//   dE  a fixed-order per-code sum in place of a scatter: the token axis is cut into S <= 32 equal segments, thread (code k, segment s)
//       walks its segment in token order and adds (z_q - z) of the tokens whose index is k; a second pass adds the S partial sums of a
//       code in segment order and scales.  No write address ever depends on an index, so an index out of range selects nothing and
//       cannot fault, and a code that owns every token costs what an unused one costs: the work is the same N / S steps for every
//       thread, which is what the split of long lists buys a gather over an inverted index (one code can own almost all tokens).
//       The price is N x K compares, the order of the forward search itself (vq.hip), 3 VALU ops each instead of its 8.
// Compiled with -ffp-contract=off like vq.hip: every rounding the error bounds of tests/test_gpu_vq_train.py count is spelled here.
#include "common.h"

namespace {

constexpr int VT_THREADS = 256;
constexpr int VT_MAX_SPANS = 1024;     // first-level sums of S
constexpr int VT_SPAN_MIN = 2048;      // elements per span at least (8 per lane)
constexpr int VT_MAX_SEGMENTS = 32;    // token segments of the per-code sum
constexpr int VT_SEGMENT_MIN = 512;    // tokens per segment at least
constexpr int VT_TILE = 512;           // tokens of a segment resident in LDS at once (x 16 B = 8 KB)

// fixed-order sum of one value per thread over a 256-thread workgroup: result valid in thread 0
__device__ __forceinline__ float block_sum_fixed(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = VT_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = __fadd_rn(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(VT_THREADS) void vq_loss_span_kernel(const float* __restrict__ z, const float* __restrict__ zq, long long n_elems,
                                                                   long long span, float* __restrict__ zst, float* __restrict__ partial) {
  __shared__ float red[VT_THREADS];
  const long long e0 = (long long)blockIdx.x * span;
  const long long e1 = e0 + span < n_elems ? e0 + span : n_elems;
  float acc = 0.f;
  for (long long e = e0 + threadIdx.x; e < e1; e += VT_THREADS) {
    const float a = z[e];
    const float d = __fsub_rn(zq[e], a);
    acc = __fadd_rn(acc, __fmul_rn(d, d));
    if (zst) zst[e] = __fadd_rn(a, d);      // z + (z_q - z): quantize.py:298, not always z_q to the bit
  }
  const float s = block_sum_fixed(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(VT_THREADS) void vq_loss_final_kernel(const float* __restrict__ partial, int n_spans, float* __restrict__ out) {
  __shared__ float red[VT_THREADS];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_spans; i += VT_THREADS) acc = __fadd_rn(acc, partial[i]);
  const float s = block_sum_fixed(acc, red);
  if (threadIdx.x == 0) out[0] = s;
}

__global__ __launch_bounds__(VT_THREADS) void vq_dz_kernel(const float* __restrict__ z, const float* __restrict__ zq, const float* __restrict__ g,
                                                            const float* __restrict__ gl, float cz, long long n_elems, float* __restrict__ dz) {
  const long long e = (long long)blockIdx.x * VT_THREADS + threadIdx.x;
  if (e >= n_elems) return;
  const float c = __fmul_rn(gl[0], cz);
  const float t = __fmul_rn(c, __fsub_rn(z[e], zq[e]));
  dz[e] = g ? __fadd_rn(g[e], t) : t;
}

// thread = one code, blockIdx.y = one token segment: partial[seg][code][3]
__global__ __launch_bounds__(VT_THREADS) void vq_de_segment_kernel(const float* __restrict__ z, const float* __restrict__ zq,
                                                                    const long long* __restrict__ idx, long long n_tokens, int n_codes,
                                                                    long long seg_len, float* __restrict__ partial) {
  __shared__ f32x4 tile[VT_TILE];
  const int code = blockIdx.x * VT_THREADS + threadIdx.x;
  const long long t0 = (long long)blockIdx.y * seg_len;
  const long long t1 = t0 + seg_len < n_tokens ? t0 + seg_len : n_tokens;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (long long base = t0; base < t1; base += VT_TILE) {
    const int nt = (int)(t1 - base < VT_TILE ? t1 - base : VT_TILE);
    __syncthreads();
    for (int t = threadIdx.x; t < nt; t += VT_THREADS) {
      const long long tok = base + t;
      const long long k = idx[tok];
      f32x4 v;
      v[0] = __fsub_rn(zq[tok * 3 + 0], z[tok * 3 + 0]);
      v[1] = __fsub_rn(zq[tok * 3 + 1], z[tok * 3 + 1]);
      v[2] = __fsub_rn(zq[tok * 3 + 2], z[tok * 3 + 2]);
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
      }
    }
  }
  if (code < n_codes) {
    float* p = partial + ((long long)blockIdx.y * n_codes + code) * 3;
    p[0] = a0;
    p[1] = a1;
    p[2] = a2;
  }
}

// thread = one element of dE: the segments' partial sums in segment order, then the scale
__global__ __launch_bounds__(VT_THREADS) void vq_de_final_kernel(const float* __restrict__ partial, int n_segments, long long n_out,
                                                                  const float* __restrict__ gl, float ce, float* __restrict__ dE) {
  const long long e = (long long)blockIdx.x * VT_THREADS + threadIdx.x;
  if (e >= n_out) return;
  float acc = partial[e];
  for (int s = 1; s < n_segments; ++s) acc = __fadd_rn(acc, partial[(long long)s * n_out + e]);
  const float r = __fmul_rn(__fmul_rn(gl[0], ce), acc);
  dE[e] = acc == 0.f ? 0.f : r;             // nothing selected the code (or its terms cancel): +0, whatever the sign of the scale
}

int n_spans(long long n_elems) {
  const long long s = cdivll(n_elems, VT_SPAN_MIN);
  return (int)(s < 1 ? 1 : (s > VT_MAX_SPANS ? VT_MAX_SPANS : s));
}

int n_segments(long long n_tokens) {
  const long long s = cdivll(n_tokens, VT_SEGMENT_MIN);
  return (int)(s < 1 ? 1 : (s > VT_MAX_SEGMENTS ? VT_MAX_SEGMENTS : s));
}

}  // namespace

extern "C" size_t glare_vq_train_workspace_bytes(long long n_tokens, int n_codes) {
  if (n_tokens <= 0 || n_codes <= 0) return 0;
  const size_t loss = (size_t)n_spans(n_tokens * 3) * sizeof(float);
  const size_t de = (size_t)n_segments(n_tokens) * (size_t)n_codes * 3 * sizeof(float);
  return loss > de ? loss : de;
}

extern "C" int glare_vq_loss_sum_f32(const float* z_nhwc, const float* zq_nhwc, long long n_tokens, int dim, float* zq_st_nhwc,
                                     float* loss_sum, void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  if (n_tokens <= 0) return GLARE_ERR_INVALID;
  if (dim != 3) return GLARE_ERR_UNSUPPORTED;
  if (!z_nhwc || !zq_nhwc || !loss_sum || !workspace) return GLARE_ERR_INVALID;
  const long long n_elems = n_tokens * 3;
  const int spans = n_spans(n_elems);
  if (workspace_bytes < (size_t)spans * sizeof(float)) return GLARE_ERR_WORKSPACE;
  const long long span = cdivll(n_elems, spans);
  float* partial = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(vq_loss_span_kernel, dim3((unsigned)spans), dim3(VT_THREADS), 0, (hipStream_t)stream, z_nhwc, zq_nhwc, n_elems, span,
                     zq_st_nhwc, partial);
  hipLaunchKernelGGL(vq_loss_final_kernel, dim3(1), dim3(VT_THREADS), 0, (hipStream_t)stream, partial, spans, loss_sum);
  return glare_launch_status();
}

extern "C" int glare_vq_backward_f32(const float* z_nhwc, const float* zq_nhwc, const long long* idx_i64, const float* g_nhwc,
                                     const float* gl_dev, long long n_tokens, int n_codes, int dim, float cz, float ce, float* dz_nhwc,
                                     float* dE, void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  if (n_tokens <= 0 || n_codes <= 0) return GLARE_ERR_INVALID;
  if (dim != 3) return GLARE_ERR_UNSUPPORTED;
  if (!z_nhwc || !zq_nhwc || !gl_dev || (!dz_nhwc && !dE)) return GLARE_ERR_INVALID;
  if (dE && (!idx_i64 || !workspace)) return GLARE_ERR_INVALID;
  const int segs = n_segments(n_tokens);
  if (dE && workspace_bytes < (size_t)segs * (size_t)n_codes * 3 * sizeof(float)) return GLARE_ERR_WORKSPACE;
  const long long n_elems = n_tokens * 3;
  if (cdivll(n_elems, VT_THREADS) > 0x7fffffffLL) return GLARE_ERR_INVALID;
  if (dz_nhwc)
    hipLaunchKernelGGL(vq_dz_kernel, dim3((unsigned)cdivll(n_elems, VT_THREADS)), dim3(VT_THREADS), 0, (hipStream_t)stream, z_nhwc, zq_nhwc,
                       g_nhwc, gl_dev, cz, n_elems, dz_nhwc);
  if (dE) {
    float* partial = reinterpret_cast<float*>(workspace);
    const long long seg_len = cdivll(n_tokens, segs);
    const long long n_out = (long long)n_codes * 3;
    hipLaunchKernelGGL(vq_de_segment_kernel, dim3((unsigned)cdiv(n_codes, VT_THREADS), (unsigned)segs), dim3(VT_THREADS), 0,
                       (hipStream_t)stream, z_nhwc, zq_nhwc, idx_i64, n_tokens, n_codes, seg_len, partial);
    hipLaunchKernelGGL(vq_de_final_kernel, dim3((unsigned)cdivll(n_out, VT_THREADS)), dim3(VT_THREADS), 0, (hipStream_t)stream, partial, segs,
                       n_out, gl_dev, ce, dE);
  }
  return glare_launch_status();
}
