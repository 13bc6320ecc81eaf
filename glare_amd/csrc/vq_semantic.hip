// The semantic guidance term of stage 1: the codes, through `conv_semantic` (1x1 conv 3 -> 256 + ReLU), are pulled towards the VGG19
// relu3_4 features of the input (reference: code/models/modules/VQModel_arch.py:85-88,
//   `emb_loss += 0.1 * F.mse_loss(self.conv_semantic(quant), vgg_feat)`; conv_semantic is built at :56-61).
// One fused pass: the loss and its three unit gradients from ONE read of the feature map; the [N][256] activation never exists.
//
//   per token t, channel c (fp32):   pre = ((W_c0 q_t0 + W_c1 q_t1) + W_c2 q_t2) + b_c     s = relu(pre)     d = s - feat_tc
//   loss  = k / 2 * sum_tc d^2                       k = 2 / (N * 256), formed in fp64 on the host and rounded to fp32 ONCE
//   e_tc  = d [pre > 0]                              (ReLU's gradient at exactly 0 is 0, as torch has it)
//   dq_tj = k * sum_c e_tc W_cj      dW_cj = k * sum_t e_tc q_tj      db_c = k * sum_t e_tc              (the gradients of `loss`)
//
// Mapping: a lane owns 4 consecutive channels, so a wave reads one token's 512-byte feature row with one 8-byte load per lane; its 12 filter
// taps, 4 biases and 16 gradient accumulators stay in registers across all the wave's tokens, q_t is wave-uniform.  A workgroup of 4 waves
// takes a run of `chunk` consecutive tokens, wave w the tokens t0 + w, t0 + w + 4, ... in ascending order, 8 loads in flight per lane.
// Sums have ONE order that depends on N alone.  No atomics:
//   dq     a lane's 4 channels in order, then the xor-shuffle tree over the wave's 64 lanes (every lane ends with the same bits), times k
//   dW, db a lane's tokens in order, the 4 waves in wave order (LDS), the workgroups (second launch), times k
//   loss   a lane's d^2 in (token, channel) order, the shuffle tree, the waves in order, the workgroups (second launch), times k / 2
// Launch 1 writes one partial row {dW[256][3], db[256], loss} per workgroup to the workspace with plain vector stores; launch 2 adds the rows:
// the workgroup axis in 8 equal slices, each in workgroup order, then the 8 slices in slice order.
// Compiled with -ffp-contract=off: every rounding the bounds of tests/test_gpu_vq_semantic.py count is spelled here.
#include "common.h"

namespace {

constexpr int VS_THREADS = 256;
constexpr int VS_WAVES = VS_THREADS / GLARE_WAVE;
constexpr int VS_COUT = 256;                       // 64 lanes x 4 channels
constexpr int VS_TILE = 64;                        // tokens per workgroup at least (16 per wave)
constexpr int VS_MAX_GROUPS = 512;                 // workgroups at most: beyond 512 x 64 tokens a workgroup's run grows instead
constexpr int VS_UNROLL = 8;                       // feature rows a wave has in flight
constexpr int VS_ROW = 3 * VS_COUT + VS_COUT + 4;  // floats of a partial row: dW | db | loss, padded to 16 bytes
constexpr int VS_SUMS = 3 * VS_COUT + VS_COUT + 1; // the sums of a row
constexpr int VS_SLICES = 8;                      // second level: slices of the workgroup axis summed side by side
constexpr int VS_FINAL_SUMS = VS_THREADS / VS_SLICES;          // ... and sums per workgroup of that launch
constexpr long long VS_MAX_TOKENS = 1ll << 24;

struct VsGeo {
  int groups;
  long long chunk;   // tokens per workgroup
};

inline VsGeo vs_geo(long long n_tokens) {
  const long long g = cdivll(n_tokens, VS_TILE);
  VsGeo q;
  q.chunk = cdivll(n_tokens, g > VS_MAX_GROUPS ? VS_MAX_GROUPS : g);
  q.groups = (int)cdivll(n_tokens, q.chunk);       // no workgroup without a token
  return q;
}

__device__ __forceinline__ float wave_sum_rn(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(VS_THREADS) void vq_semantic_kernel(const float* __restrict__ quant, const float* __restrict__ weight,
                                                                 const float* __restrict__ bias, const a16_t* __restrict__ feat,
                                                                 long long n_tokens, long long chunk, float k, float* __restrict__ dq,
                                                                 float* __restrict__ partial) {
  __shared__ float red[VS_WAVES][VS_ROW];
  const int lane = threadIdx.x & (GLARE_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / GLARE_WAVE);
  const int c0 = lane * 4;
  float w[4][3], b[4], dw[4][3], db[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    b[i] = bias[c0 + i];
    db[i] = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      w[i][j] = weight[(c0 + i) * 3 + j];
      dw[i][j] = 0.f;
    }
  }
  float lsum = 0.f;
  const long long t0 = (long long)blockIdx.x * chunk;
  const long long t1 = t0 + chunk < n_tokens ? t0 + chunk : n_tokens;     // t0 < n_tokens: vs_geo leaves no workgroup without a token
  for (long long base = t0 + wave; base < t1; base += VS_WAVES * VS_UNROLL) {
    u32x2 r[VS_UNROLL];
    float qv[VS_UNROLL][3];
#pragma unroll
    for (int u = 0; u < VS_UNROLL; ++u) {          // all of the round's loads first; a slot past the run re-reads the run's last token
      const long long t = base + u * VS_WAVES < t1 ? base + u * VS_WAVES : t1 - 1;
      r[u] = *reinterpret_cast<const u32x2*>(feat + t * VS_COUT + c0);
#pragma unroll
      for (int j = 0; j < 3; ++j) qv[u][j] = quant[t * 3 + j];
    }
#pragma unroll
    for (int u = 0; u < VS_UNROLL; ++u) {
      const long long t = base + u * VS_WAVES;
      if (t < t1) {                                // wave-uniform
        const float f[4] = {alo(r[u][0]), ahi(r[u][0]), alo(r[u][1]), ahi(r[u][1])};
        float p[3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // pre: 3 products + 3 sums = 6 roundings
          const float pre = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w[i][0], qv[u][0]), __fmul_rn(w[i][1], qv[u][1])), __fmul_rn(w[i][2], qv[u][2])), b[i]);
          const float s = pre < 0.f ? 0.f : pre;   // (a NaN stays a NaN)
          const float d = __fsub_rn(s, f[i]);      // 1 rounding
          lsum = __fadd_rn(lsum, __fmul_rn(d, d)); // 1 rounding for the square, 1 per add of the lane's chain
          const float e = pre > 0.f ? d : 0.f;
          db[i] = __fadd_rn(db[i], e);             // 1 per token of the wave
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            dw[i][j] = __fadd_rn(dw[i][j], __fmul_rn(e, qv[u][j]));       // 1 for the product, 1 per token of the wave
            const float ew = __fmul_rn(e, w[i][j]);                         // 1
            p[j] = i == 0 ? ew : __fadd_rn(p[j], ew);                       // 3 for the lane's 4 channels
          }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) p[j] = wave_sum_rn(p[j]);              // 6
        if (lane < 3) dq[t * 3 + lane] = __fmul_rn(k, lane == 0 ? p[0] : (lane == 1 ? p[1] : p[2]));     // 1 (+ 1: k itself is rounded)
      }
    }
  }
  lsum = wave_sum_rn(lsum);                        // 6
  float* row = red[wave];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) row[(c0 + i) * 3 + j] = dw[i][j];
    row[3 * VS_COUT + c0 + i] = db[i];
  }
  if (lane == 0) row[4 * VS_COUT] = lsum;
  __syncthreads();
  float* out = partial + (long long)blockIdx.x * VS_ROW;
  for (int e = threadIdx.x; e < VS_SUMS; e += VS_THREADS)
    out[e] = __fadd_rn(__fadd_rn(__fadd_rn(red[0][e], red[1][e]), red[2][e]), red[3][e]);            // 3: the waves in wave order
}
static_assert(VS_WAVES == 4, "the workgroup's sum is written out for four waves");

// The second level.  A workgroup = 32 of the 1025 sums x 8 slices of the workgroup axis: thread (sum e, slice s) adds the partial rows of
// workgroups [s L, (s + 1) L), L = ceil(groups / 8), in workgroup order (its loads are independent: 16 in flight), then thread (e, 0) adds
// the 8 slices in slice order (LDS) -- at most L - 1 + 7 roundings --, then the factor (1, + 1 for k).  An empty slice adds +0.
__global__ __launch_bounds__(VS_THREADS) void vq_semantic_final_kernel(const float* __restrict__ partial, int groups, float k,
                                                                       float* __restrict__ loss, float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float red[VS_SLICES][VS_FINAL_SUMS];
  const int col = threadIdx.x % VS_FINAL_SUMS, slice = threadIdx.x / VS_FINAL_SUMS;
  const int e = blockIdx.x * VS_FINAL_SUMS + col;
  const int per = (groups + VS_SLICES - 1) / VS_SLICES;
  const int g0 = slice * per, g1 = g0 + per < groups ? g0 + per : groups;
  float acc = 0.f;
  if (e < VS_SUMS && g0 < g1) {
    acc = partial[(long long)g0 * VS_ROW + e];
#pragma unroll 16
    for (int g = g0 + 1; g < g1; ++g) acc = __fadd_rn(acc, partial[(long long)g * VS_ROW + e]);
  }
  red[slice][col] = acc;
  __syncthreads();
  if (slice != 0 || e >= VS_SUMS) return;
  acc = red[0][col];
#pragma unroll
  for (int s = 1; s < VS_SLICES; ++s) acc = __fadd_rn(acc, red[s][col]);
  if (e < 3 * VS_COUT)
    dW[e] = __fmul_rn(k, acc);
  else if (e < 4 * VS_COUT)
    db[e - 3 * VS_COUT] = __fmul_rn(k, acc);
  else
    loss[0] = __fmul_rn(0.5f * k, acc);            // (the halving is exact)
}

// out = g * unit over the three gradients in one launch: element i of dq [n_dq], then dW [768], then db [256]
__global__ __launch_bounds__(VS_THREADS) void vq_semantic_scale_kernel(const float* __restrict__ g_dev, long long n_dq, const float* __restrict__ dq_unit,
                                                                       const float* __restrict__ dW_unit, const float* __restrict__ db_unit,
                                                                       float* __restrict__ dq, float* __restrict__ dW, float* __restrict__ db) {
  const long long i = (long long)blockIdx.x * VS_THREADS + threadIdx.x;
  const float g = g_dev[0];
  if (i < n_dq) {
    if (dq) dq[i] = __fmul_rn(g, dq_unit[i]);
  } else if (i < n_dq + 3 * VS_COUT) {
    if (dW) dW[i - n_dq] = __fmul_rn(g, dW_unit[i - n_dq]);
  } else if (i < n_dq + 4 * VS_COUT) {
    if (db) db[i - n_dq - 3 * VS_COUT] = __fmul_rn(g, db_unit[i - n_dq - 3 * VS_COUT]);
  }
}

}  // namespace

extern "C" size_t glare_vq_semantic_workspace_bytes(long long n_tokens, int cout) {
  if (n_tokens <= 0 || n_tokens > VS_MAX_TOKENS || cout != VS_COUT) return 0;
  return (size_t)vs_geo(n_tokens).groups * VS_ROW * sizeof(float);
}

extern "C" int glare_vq_semantic_bf16(const float* quant, const float* weight, const float* bias, const void* feat, long long n_tokens, int cout,
                                      float* loss_out, float* dq, float* dW, float* db, void* workspace, size_t workspace_bytes,
                                      glare_stream_t stream) {
  if (n_tokens <= 0 || cout <= 0) return GLARE_ERR_INVALID;
  if (!quant || !weight || !bias || !feat || !loss_out || !dq || !dW || !db) return GLARE_ERR_INVALID;
  if (((uintptr_t)feat & 7u) != 0 || ((uintptr_t)workspace & 3u) != 0) return GLARE_ERR_INVALID;
  if (cout != VS_COUT || n_tokens > VS_MAX_TOKENS) return GLARE_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < glare_vq_semantic_workspace_bytes(n_tokens, cout)) return GLARE_ERR_WORKSPACE;
  const VsGeo q = vs_geo(n_tokens);
  const float k = (float)(2.0 / ((double)n_tokens * VS_COUT));
  float* partial = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(vq_semantic_kernel, dim3((unsigned)q.groups), dim3(VS_THREADS), 0, s, quant, weight, bias, static_cast<const a16_t*>(feat),
                     n_tokens, q.chunk, k, dq, partial);
  hipLaunchKernelGGL(vq_semantic_final_kernel, dim3((unsigned)cdiv(VS_SUMS, VS_FINAL_SUMS)), dim3(VS_THREADS), 0, s, partial, q.groups, k, loss_out,
                     dW, db);
  return glare_launch_status();
}

extern "C" int glare_vq_semantic_scale_f32(const float* g_dev, long long n_tokens, const float* dq_unit, const float* dW_unit,
                                           const float* db_unit, float* dq, float* dW, float* db, glare_stream_t stream) {
  if (n_tokens <= 0) return GLARE_ERR_INVALID;
  if (!g_dev || !dq_unit || (dW && !dW_unit) || (db && !db_unit) || !dq) return GLARE_ERR_INVALID;
  if (n_tokens > VS_MAX_TOKENS) return GLARE_ERR_UNSUPPORTED;
  const long long n = n_tokens * 3 + 4 * VS_COUT;
  hipLaunchKernelGGL(vq_semantic_scale_kernel, dim3((unsigned)cdivll(n, VS_THREADS)), dim3(VS_THREADS), 0, (hipStream_t)stream, g_dev,
                     n_tokens * 3, dq_unit, dW_unit, db_unit, dq, dW, db);
  return glare_launch_status();
}
