// Exponential moving average of the trained weights, and the in-place exchange that lets validation run under it.
//
// Replaces BaseModel.model_ema (reference lineage: basicsr/models/base_model.py:85-92, `net_g_ema = decay * net_g_ema + (1 - decay) * net_g`
// over every parameter, one torch op each) with ONE streaming launch per flat parameter buffer (train.FlatGroup.w).  Semantics:
// include/glare_hip.h.
//   glare_weight_ema_f32   *seeded == 0: ema = w (bit copy);  else ema = fmaf(decay, ema, one_minus_decay * w)
//   glare_swap_f32         a <-> b
//
// Both are bandwidth-bound (12 and 16 bytes per element) and share one shape: 256-thread workgroups, a thread moves one 16-byte vector per
// trip, grid = min(ceil(vectors / 256), 2048) workgroups (8 per CU: 8 waves per SIMD in flight) and a grid-stride loop for the rest.  The
// FIRST pointer (the one read and written) sets the vector phase: up to 3 leading elements bring it to a 16-byte boundary and up to 3
// trail the last whole vector; threads 0..2 of workgroup 0 take those one element each.  The second pointer is read / written as vectors
// when it shares that phase and as 4 dwords per vector when it does not (slices of the flat buffers are only 4-byte aligned).
// The roundings are spelled: the product one_minus_decay * w is its own operation and fmaf() is one more; no contraction can merge them
// (fmaf already is the fused form).  Plain vector loads and stores only; the seeded flag is read, never written.
#include "common.h"

namespace {

constexpr int WE_THREADS = 256;
constexpr long long WE_MAX_BLOCKS = 2048;   // 256 CUs x 8 workgroups

struct Split {      // n elements at p = head (< 4) + 4 * nvec + tail (< 4), the vectors 16-byte aligned
  int head, tail;
  long long nvec;
};

Split split_at(const void* p, long long n) {
  Split s;
  const long long lead = (long long)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 4);
  s.head = (int)(lead < n ? lead : n);
  s.nvec = (n - s.head) / 4;
  s.tail = (int)(n - s.head - 4 * s.nvec);
  return s;
}

unsigned grid_for(long long nvec) {
  const long long b = cdivll(nvec, WE_THREADS);
  return (unsigned)(b < 1 ? 1 : (b > WE_MAX_BLOCKS ? WE_MAX_BLOCKS : b));
}

template <bool VEC>
__device__ __forceinline__ float4 load4(const float* p, long long i) {
  if (VEC) return reinterpret_cast<const float4*>(p)[i];
  return make_float4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]);
}

template <bool VEC>
__device__ __forceinline__ void store4(float* p, long long i, float4 v) {
  if (VEC) {
    reinterpret_cast<float4*>(p)[i] = v;
  } else {
    p[4 * i] = v.x; p[4 * i + 1] = v.y; p[4 * i + 2] = v.z; p[4 * i + 3] = v.w;
  }
}

__device__ __forceinline__ float ema1(float d, float e, float omd, float x) { return fmaf(d, e, omd * x); }

// W_VEC: w + head is 16-byte aligned too
template <bool W_VEC>
__global__ __launch_bounds__(WE_THREADS) void weight_ema_kernel(float* ema, const float* __restrict__ w, int head, long long nvec, int tail,
                                                               float d, float omd, const int* __restrict__ seeded) {
  const bool seed = *seeded == 0;     // uniform across the launch (a scalar load)
  if (blockIdx.x == 0 && threadIdx.x < 3) {
    const int t = threadIdx.x;
    if (t < head) ema[t] = seed ? w[t] : ema1(d, ema[t], omd, w[t]);
    if (t < tail) {
      const long long i = head + 4 * nvec + t;
      ema[i] = seed ? w[i] : ema1(d, ema[i], omd, w[i]);
    }
  }
  float* eb = ema + head;
  const float* wb = w + head;
  const long long stride = (long long)gridDim.x * WE_THREADS;
  if (seed) {                         // the first step: a copy, ema (uninitialised) is not read
    for (long long i = (long long)blockIdx.x * WE_THREADS + threadIdx.x; i < nvec; i += stride) store4<true>(eb, i, load4<W_VEC>(wb, i));
    return;
  }
  for (long long i = (long long)blockIdx.x * WE_THREADS + threadIdx.x; i < nvec; i += stride) {
    const float4 x = load4<W_VEC>(wb, i);
    float4 e = load4<true>(eb, i);
    e.x = ema1(d, e.x, omd, x.x);
    e.y = ema1(d, e.y, omd, x.y);
    e.z = ema1(d, e.z, omd, x.z);
    e.w = ema1(d, e.w, omd, x.w);
    store4<true>(eb, i, e);
  }
}

template <bool B_VEC>
__global__ __launch_bounds__(WE_THREADS) void swap_kernel(float* __restrict__ a, float* __restrict__ b, int head, long long nvec, int tail) {
  if (blockIdx.x == 0 && threadIdx.x < 3) {
    const int t = threadIdx.x;
    if (t < head) { const float x = a[t]; a[t] = b[t]; b[t] = x; }
    if (t < tail) {
      const long long i = head + 4 * nvec + t;
      const float x = a[i]; a[i] = b[i]; b[i] = x;
    }
  }
  float* ab = a + head;
  float* bb = b + head;
  const long long stride = (long long)gridDim.x * WE_THREADS;
  for (long long i = (long long)blockIdx.x * WE_THREADS + threadIdx.x; i < nvec; i += stride) {
    const float4 x = load4<true>(ab, i);
    const float4 y = load4<B_VEC>(bb, i);
    store4<true>(ab, i, y);
    store4<B_VEC>(bb, i, x);
  }
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

#define ST(s) static_cast<hipStream_t>(s)

extern "C" int glare_weight_ema_f32(float* ema, const float* w, long long n, float decay, float one_minus_decay, const int* seeded_device,
                                    glare_stream_t stream) {
  if (n < 0 || !(decay >= 0.f && decay < 1.f)) return GLARE_ERR_INVALID;      // (a NaN decay fails the comparison)
  if (n == 0) return GLARE_OK;
  if (!ema || !w || !seeded_device || !aligned4(ema) || !aligned4(w)) return GLARE_ERR_INVALID;
  const Split s = split_at(ema, n);
  if (aligned16(w + s.head))
    hipLaunchKernelGGL(weight_ema_kernel<true>, dim3(grid_for(s.nvec)), dim3(WE_THREADS), 0, ST(stream), ema, w, s.head, s.nvec, s.tail,
                       decay, one_minus_decay, seeded_device);
  else
    hipLaunchKernelGGL(weight_ema_kernel<false>, dim3(grid_for(s.nvec)), dim3(WE_THREADS), 0, ST(stream), ema, w, s.head, s.nvec, s.tail,
                       decay, one_minus_decay, seeded_device);
  return glare_launch_status();
}

extern "C" int glare_swap_f32(float* a, float* b, long long n, glare_stream_t stream) {
  if (n < 0) return GLARE_ERR_INVALID;
  if (n == 0) return GLARE_OK;
  if (!a || !b || !aligned4(a) || !aligned4(b)) return GLARE_ERR_INVALID;
  if (a < b + n && b < a + n) return GLARE_ERR_INVALID;                       // overlapping ranges (a == b included)
  const Split s = split_at(a, n);
  if (aligned16(b + s.head))
    hipLaunchKernelGGL(swap_kernel<true>, dim3(grid_for(s.nvec)), dim3(WE_THREADS), 0, ST(stream), a, b, s.head, s.nvec, s.tail);
  else
    hipLaunchKernelGGL(swap_kernel<false>, dim3(grid_for(s.nvec)), dim3(WE_THREADS), 0, ST(stream), a, b, s.head, s.nvec, s.tail);
  return glare_launch_status();
}
