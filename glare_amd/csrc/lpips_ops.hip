// The LPIPS perceptual term of stage 1 (taming's VQLPIPSWithDiscriminator: nll = |x - xrec| + perceptual_weight * LPIPS_vgg(x, xrec), behind
// `self.loss(...)` of VQModel.training_step, code/models/modules/VQModel_arch.py:110-160): the head of ONE feature tap, forward and backward,
// on the 16-bit NHWC feature maps of the training path, and the ScalingLayer in front of the trunk.  The trunk's convolutions run on
// conv_igemm.hip, its pools on loss_ops.hip.
//
//   per pixel (fp32):   na = sqrt(sum_c a_c^2)   nb = sqrt(sum_c b_c^2)   ah = a / (na + eps)   bh = b / (nb + eps)
//   per image i:        out[i] = (1 / HW) sum_pixels sum_c w_c (ah_c - bh_c)^2
//   backward (a only):  e_c = 2 w_c (ah_c - bh_c)    s = sum_c e_c a_c
//                       da_c = (g[i] / HW) (e_c / (na + eps) - a_c s / (na (na + eps)^2))          stored 16-bit, rounded ONCE
//   a pixel of `a` that is all zero: da = 0 for every channel (the forward value stays the finite one, ah = 0).  autograd returns NaN there
//   (0 * inf in sqrt's backward) and the analytic derivative is of order 1 / eps: the one deliberate deviation.
//
// Streaming kernels: a pixel's C channels are contiguous; a lane loads 16 B (8 channels) of a and of b, C / 8 = 8 .. 64 consecutive lanes
// hold one pixel and reduce over it with xor-shuffles inside their own aligned group (every lane of the group ends with the same bits).
// The backward recomputes na, nb and s: it reads a and b once, writes da, and nothing pixel-sized is saved by the forward.
// Sums have ONE order that depends on the shape alone: a lane's 8 channels in order, the shuffle tree, a group's pixels in ascending order,
// the groups of a workgroup in group order (thread 0), the workgroups of an image through one halving tree in LDS (second launch).  No atomics.
// Compiled with -ffp-contract=off: every rounding the bounds of tests/test_gpu_lpips_kernels.py count is spelled here.
#include "common.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_MAX_CHUNKS = 256;   // workgroups per image at most
constexpr int LP_CHUNK_ITERS = 4;    // a workgroup walks at least this many rounds of its pixels-per-round before an image is cut further

struct LpGeo {
  long long HW;
  long long chunk;   // pixels per workgroup (forward)
  int C, L, PPB, S;  // lanes per pixel, pixels per workgroup round, workgroups per image
};

inline LpGeo lp_geo(long long HW, int C) {
  LpGeo q;
  q.HW = HW;
  q.C = C;
  q.L = C / 8;
  q.PPB = LP_THREADS / q.L;
  const long long s = cdivll(HW, (long long)q.PPB * LP_CHUNK_ITERS);
  q.S = (int)(s < 1 ? 1 : (s > LP_MAX_CHUNKS ? LP_MAX_CHUNKS : s));
  q.chunk = cdivll(HW, q.S);
  return q;
}

struct Px8 {
  float v[8];
};

__device__ __forceinline__ Px8 load8(const a16_t* p) {
  const u32x4 r = *reinterpret_cast<const u32x4*>(p);
  Px8 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    o.v[2 * k] = alo(r[k]);
    o.v[2 * k + 1] = ahi(r[k]);
  }
  return o;
}

// sum over the L lanes of a pixel's aligned group; L a power of two in [8, 64]
__device__ __forceinline__ float group_sum(float v, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float sumsq8(const Px8& x) {
  float q = __fmul_rn(x.v[0], x.v[0]);
#pragma unroll
  for (int k = 1; k < 8; ++k) q = __fadd_rn(q, __fmul_rn(x.v[k], x.v[k]));
  return q;
}

// partial[(img * S + s)] = sum over the workgroup's pixels of sum_c w_c (ah_c - bh_c)^2
__global__ __launch_bounds__(LP_THREADS) void lpips_head_fwd_kernel(const a16_t* __restrict__ a, const a16_t* __restrict__ b, const float* __restrict__ w,
                                                                    const LpGeo q, float eps, float* __restrict__ partial) {
  __shared__ float red[LP_THREADS / 8];
  const int lane = threadIdx.x % q.L, grp = threadIdx.x / q.L;
  const int img = blockIdx.y, s = blockIdx.x;
  const long long p0 = (long long)s * q.chunk, p1 = p0 + q.chunk < q.HW ? p0 + q.chunk : q.HW;
  float wv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) wv[k] = w[lane * 8 + k];
  float acc = 0.f;
  // (the trip count is the same for every lane of a group: the shuffles inside see whole groups; groups of one wave may differ by one
  //  round, and a lane past its last pixel only lends its registers to nobody -- the xor partners stay inside the group)
  for (long long pix = p0 + grp; pix < p1; pix += q.PPB) {
    const long long off = ((long long)img * q.HW + pix) * q.C + lane * 8;
    const Px8 xa = load8(a + off), xb = load8(b + off);
    const float na = sqrtf(group_sum(sumsq8(xa), q.L)), nb = sqrtf(group_sum(sumsq8(xb), q.L));
    const float ia = 1.0f / __fadd_rn(na, eps), ib = 1.0f / __fadd_rn(nb, eps);
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float d = __fsub_rn(__fmul_rn(xa.v[k], ia), __fmul_rn(xb.v[k], ib));
      const float u = __fmul_rn(__fmul_rn(wv[k], d), d);
      t = k == 0 ? u : __fadd_rn(t, u);
    }
    acc = __fadd_rn(acc, group_sum(t, q.L));
  }
  if (lane == 0) red[grp] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = red[0];
    for (int k = 1; k < q.PPB; ++k) tot = __fadd_rn(tot, red[k]);
    partial[(long long)img * q.S + s] = tot;
  }
}

// workgroup = one image: its workgroups' partial sums (S <= LP_THREADS, the rest of the tree's leaves are 0) through a halving tree in LDS
// whose shape is LP_THREADS' alone, then the spatial mean
static_assert(LP_MAX_CHUNKS <= LP_THREADS, "the second stage holds one partial sum per thread");
__global__ __launch_bounds__(LP_THREADS) void lpips_head_final_kernel(const float* __restrict__ partial, int S, float hw, float* __restrict__ out) {
  __shared__ float red[LP_THREADS];
  const int img = blockIdx.x, t = threadIdx.x;
  red[t] = t < S ? partial[(long long)img * S + t] : 0.f;
  __syncthreads();
  for (int o = LP_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] = __fadd_rn(red[t], red[t + o]);
    __syncthreads();
  }
  if (t == 0) out[img] = red[0] / hw;
}

__global__ __launch_bounds__(LP_THREADS) void lpips_head_bwd_kernel(const a16_t* __restrict__ a, const a16_t* __restrict__ b, const float* __restrict__ w,
                                                                    const LpGeo q, long long n_pixels, float eps, float hw, const float* __restrict__ g,
                                                                    a16_t* __restrict__ da) {
  const int lane = threadIdx.x % q.L, grp = threadIdx.x / q.L;
  const long long pix = (long long)blockIdx.x * q.PPB + grp;       // over all images; the same for every lane of a group
  if (pix >= n_pixels) return;                                     // whole groups leave: the shuffles below see complete groups only
  const long long off = pix * q.C + lane * 8;
  const Px8 xa = load8(a + off), xb = load8(b + off);
  const float na = sqrtf(group_sum(sumsq8(xa), q.L)), nb = sqrtf(group_sum(sumsq8(xb), q.L));
  const float den1 = __fadd_rn(na, eps);
  const float ia = 1.0f / den1, ib = 1.0f / __fadd_rn(nb, eps);
  float e[8], t = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float d = __fsub_rn(__fmul_rn(xa.v[k], ia), __fmul_rn(xb.v[k], ib));
    e[k] = __fmul_rn(2.0f * w[lane * 8 + k], d);                   // (the doubling is exact)
    const float u = __fmul_rn(e[k], xa.v[k]);
    t = k == 0 ? u : __fadd_rn(t, u);
  }
  const float s = group_sum(t, q.L);
  const float gs = g[pix / q.HW] / hw;
  const float kk = s / __fmul_rn(na, __fmul_rn(den1, den1));         // na = 0: 0 / 0, never used (the select below)
  const bool zero = !(na > 0.f);
  float r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float v = __fmul_rn(gs, __fsub_rn(__fmul_rn(e[k], ia), __fmul_rn(xa.v[k], kk)));
    r[k] = zero ? 0.f : v;
  }
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = pack_a2(r[2 * k], r[2 * k + 1]);
  *reinterpret_cast<u32x4*>(da + off) = o;
}

// y[p][c] = x[p][c] * mul[c] (+ add[c])
__global__ __launch_bounds__(LP_THREADS) void image_affine_kernel(const float* __restrict__ x, const float* __restrict__ mul, const float* __restrict__ add,
                                                                  float* __restrict__ y, long long n, int C) {
  const long long i = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % C);
  y[i] = add ? fmaf(x[i], mul[c], add[c]) : __fmul_rn(x[i], mul[c]);
}

inline int lp_check(int B, long long HW, int C) {
  if (B <= 0 || HW <= 0 || C <= 0 || C % 8 != 0) return GLARE_ERR_INVALID;
  if (C != 64 && C != 128 && C != 256 && C != 512) return GLARE_ERR_UNSUPPORTED;        // a pixel = a power-of-two group of 8 .. 64 lanes
  if (B > 65535 || HW >= (1ll << 24)) return GLARE_ERR_UNSUPPORTED;                      // grid.y; (float)HW exact
  if (cdivll((long long)B * HW, LP_THREADS / (C / 8)) > 0x7fffffffLL) return GLARE_ERR_UNSUPPORTED;
  return GLARE_OK;
}

}  // namespace

#define ST(s) static_cast<hipStream_t>(s)

extern "C" size_t glare_lpips_head_workspace_bytes(int B, long long HW, int C) {
  if (lp_check(B, HW, C) != GLARE_OK) return 0;
  return (size_t)B * lp_geo(HW, C).S * sizeof(float);
}

extern "C" int glare_lpips_head_bf16(const void* a, const void* b, const float* w, int B, long long HW, int C, float eps, float* out,
                                     void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  const int rc = lp_check(B, HW, C);
  if (rc != GLARE_OK) return rc;
  if (!a || !b || !w || !out || !(eps > 0.f)) return GLARE_ERR_INVALID;
  if (!workspace || workspace_bytes < glare_lpips_head_workspace_bytes(B, HW, C)) return GLARE_ERR_WORKSPACE;
  const LpGeo q = lp_geo(HW, C);
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(lpips_head_fwd_kernel, dim3((unsigned)q.S, (unsigned)B), dim3(LP_THREADS), 0, ST(stream), static_cast<const a16_t*>(a),
                     static_cast<const a16_t*>(b), w, q, eps, partial);
  hipLaunchKernelGGL(lpips_head_final_kernel, dim3((unsigned)B), dim3(LP_THREADS), 0, ST(stream), partial, q.S, (float)HW, out);
  return glare_launch_status();
}

extern "C" int glare_lpips_head_backward_bf16(const void* a, const void* b, const float* w, int B, long long HW, int C, float eps, const float* g,
                                              void* grad_a, glare_stream_t stream) {
  const int rc = lp_check(B, HW, C);
  if (rc != GLARE_OK) return rc;
  if (!a || !b || !w || !g || !grad_a || !(eps > 0.f)) return GLARE_ERR_INVALID;
  const LpGeo q = lp_geo(HW, C);
  const long long n_pixels = (long long)B * HW;
  hipLaunchKernelGGL(lpips_head_bwd_kernel, dim3((unsigned)cdivll(n_pixels, q.PPB)), dim3(LP_THREADS), 0, ST(stream), static_cast<const a16_t*>(a),
                     static_cast<const a16_t*>(b), w, q, n_pixels, eps, (float)HW, g, static_cast<a16_t*>(grad_a));
  return glare_launch_status();
}

extern "C" int glare_image_affine_f32(const float* x, const float* mul, const float* add_or_null, float* y, long long n_pixels, int C,
                                      glare_stream_t stream) {
  if (n_pixels < 0 || C <= 0) return GLARE_ERR_INVALID;
  if (n_pixels == 0) return GLARE_OK;
  if (!x || !mul || !y) return GLARE_ERR_INVALID;
  if ((double)n_pixels * C >= 9.0e18 || cdivll(n_pixels * C, LP_THREADS) > 0x7fffffffLL) return GLARE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(image_affine_kernel, dim3((unsigned)cdivll(n_pixels * C, LP_THREADS)), dim3(LP_THREADS), 0, ST(stream), x, mul, add_or_null, y,
                     n_pixels * C, C);
  return glare_launch_status();
}
