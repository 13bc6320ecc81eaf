// Codebook usage: how many tokens select each code, and the statistics of such a histogram.
//
// The reference's VectorQuantizer2 returns perplexity = None (code/models/modules/quantize.py:286); its older VectorQuantizer computes
//   e_mean = mean over tokens of one_hot(idx);  perplexity = exp(-sum_k e_mean_k * log(e_mean_k + 1e-10))      (quantize.py:83-85)
// and basicsr/active_codebook.py counts index use over a test set.  Both are a histogram of the indices glare_vq_nearest_f32 wrote:
//   glare_vq_usage_i64    idx [G][n] -> counts [G][K] (one row per group = one image's latent), out_of_range [G], total [K] += sum_g counts
//   glare_vq_usage_stats  rows [R][K] -> tokens, active (codes with count > 0), entropy, perplexity per row, fp64 from the exact counts
//
// Everything is an exact integer up to the fp64 statistics, and bitwise the same on every run:
//   pass 1  workgroup (span s, code tier p, group g) histograms the tokens [s * span, (s + 1) * span) of group g whose index lies in
//           [p * VU_TIER, (p + 1) * VU_TIER) in LDS with integer LDS adds -- integer addition is associative, the arrival order cannot
//           change a count -- and writes its row of 32-bit partial counts with plain stores.  An index outside [0, K) is counted by the
//           tier-0 workgroup of its span and selects nothing: the only index-dependent address is hist[v - k0] behind 0 <= v - k0 < tier.
//   pass 2  thread k adds the partial rows of code k in (group, span) order, writes counts[g][k] and adds the sum over g to total[k].
// No global atomics, no float atomics.  K <= VU_TIER is one tier (32 KB of LDS at K = 8192); a larger K re-reads the indices once per tier.
// The statistics: one workgroup per row; tokens and active are integer sums, the entropy's K terms p log(p + 1e-10) are formed in fp64,
// each lane adding its strided sub-sequence in ascending order, then a fixed LDS tree.  Compiled with -ffp-contract=off.
#include "common.h"

namespace {

constexpr int VU_THREADS = 256;
constexpr int VU_TIER = GLARE_VQ_USAGE_TIER;          // codes a workgroup histograms at once (x 4 B of LDS)
constexpr int VU_SPAN = GLARE_VQ_USAGE_SPAN;          // tokens per span at least
constexpr int VU_MAX_SPANS = 64;                      // spans per group at most (the partial rows of the workspace)

inline int n_spans(long long n) {
  const long long s = cdivll(n, VU_SPAN);
  return (int)(s < 1 ? 1 : (s > VU_MAX_SPANS ? VU_MAX_SPANS : s));
}

__global__ __launch_bounds__(VU_THREADS) void vq_usage_hist_kernel(const long long* __restrict__ idx, long long n, int K, long long span,
                                                                   unsigned* __restrict__ partial, unsigned* __restrict__ oor_partial) {
  __shared__ unsigned hist[VU_TIER];
  __shared__ unsigned oor_s;
  const int s = blockIdx.x, p = blockIdx.y, g = blockIdx.z, S = gridDim.x;
  const long long k0 = (long long)p * VU_TIER;
  const int kt = (int)((long long)K - k0 < VU_TIER ? (long long)K - k0 : VU_TIER);
  for (int k = threadIdx.x; k < kt; k += VU_THREADS) hist[k] = 0u;
  if (threadIdx.x == 0) oor_s = 0u;
  __syncthreads();
  long long e0 = (long long)s * span, e1 = e0 + span;
  if (e1 > n) e1 = n;
  const long long* row = idx + (long long)g * n;
  unsigned oor = 0u;
  for (long long e = e0 + threadIdx.x; e < e1; e += VU_THREADS) {
    const long long v = row[e];
    if (v < 0 || v >= (long long)K) {
      ++oor;
    } else {
      const long long r = v - k0;
      if (r >= 0 && r < (long long)kt) atomicAdd(&hist[(int)r], 1u);      // LDS integer add
    }
  }
  if (p == 0 && oor) atomicAdd(&oor_s, oor);
  __syncthreads();
  unsigned* out = partial + ((size_t)g * S + s) * (size_t)K + (size_t)k0;
  for (int k = threadIdx.x; k < kt; k += VU_THREADS) out[k] = hist[k];
  if (p == 0 && threadIdx.x == 0) oor_partial[(size_t)g * S + s] = oor_s;
}

__global__ __launch_bounds__(VU_THREADS) void vq_usage_sum_kernel(const unsigned* __restrict__ partial, const unsigned* __restrict__ oor_partial,
                                                                  int G, int S, int K, long long* __restrict__ counts,
                                                                  long long* __restrict__ out_of_range, long long* __restrict__ total) {
  const int k = blockIdx.x * VU_THREADS + threadIdx.x;
  if (k < K) {
    long long tot = 0;
    for (int g = 0; g < G; ++g) {
      long long c = 0;
      for (int s = 0; s < S; ++s) c += (long long)partial[((size_t)g * S + s) * (size_t)K + k];
      counts[(size_t)g * K + k] = c;
      tot += c;
    }
    if (total) total[k] += tot;
  }
  if (blockIdx.x == 0)
    for (int g = threadIdx.x; g < G; g += VU_THREADS) {
      long long c = 0;
      for (int s = 0; s < S; ++s) c += (long long)oor_partial[(size_t)g * S + s];
      out_of_range[g] = c;
    }
}

__global__ __launch_bounds__(VU_THREADS) void vq_usage_stats_kernel(const long long* __restrict__ counts, int K, long long* __restrict__ tokens,
                                                                    long long* __restrict__ active, double* __restrict__ entropy,
                                                                    double* __restrict__ perplexity) {
  __shared__ long long red_t[VU_THREADS], red_a[VU_THREADS];
  __shared__ double red_d[VU_THREADS];
  const long long* row = counts + (size_t)blockIdx.x * K;
  long long t = 0, a = 0;
  for (int k = threadIdx.x; k < K; k += VU_THREADS) {
    const long long c = row[k];
    t += c;
    a += c > 0 ? 1 : 0;
  }
  red_t[threadIdx.x] = t;
  red_a[threadIdx.x] = a;
  __syncthreads();
  for (int o = VU_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red_t[threadIdx.x] += red_t[threadIdx.x + o];
      red_a[threadIdx.x] += red_a[threadIdx.x + o];
    }
    __syncthreads();
  }
  const long long n_tok = red_t[0];
  double acc = 0.0;
  if (n_tok > 0) {
    const double n_d = (double)n_tok;
    for (int k = threadIdx.x; k < K; k += VU_THREADS) {
      const double p = (double)row[k] / n_d;
      acc = acc + p * log(p + 1e-10);               // quantize.py:85, in fp64
    }
  }
  red_d[threadIdx.x] = acc;
  __syncthreads();
  for (int o = VU_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red_d[threadIdx.x] = red_d[threadIdx.x] + red_d[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double h = 0.0 - red_d[0];                // a row without tokens: the sum is empty, entropy 0, perplexity exp(0) = 1
    tokens[blockIdx.x] = n_tok;
    active[blockIdx.x] = red_a[0];
    entropy[blockIdx.x] = h;
    perplexity[blockIdx.x] = exp(h);
  }
}

}  // namespace

extern "C" size_t glare_vq_usage_workspace_bytes(int groups, long long n_tokens, int n_codes) {
  if (groups <= 0 || n_tokens <= 0 || n_codes <= 0 || n_codes > GLARE_VQ_USAGE_MAX_CODES) return 0;
  return (size_t)groups * (size_t)n_spans(n_tokens) * ((size_t)n_codes + 1) * sizeof(unsigned);
}

extern "C" int glare_vq_usage_i64(const long long* idx_i64, int groups, long long n_tokens, int n_codes, long long* counts,
                                  long long* out_of_range, long long* total, void* workspace, size_t workspace_bytes,
                                  glare_stream_t stream) {
  if (groups <= 0 || n_tokens <= 0 || n_codes <= 0) return GLARE_ERR_INVALID;
  if (!idx_i64 || !counts || !out_of_range || !workspace) return GLARE_ERR_INVALID;
  if (n_codes > GLARE_VQ_USAGE_MAX_CODES || groups > 65535) return GLARE_ERR_UNSUPPORTED;
  const int S = n_spans(n_tokens);
  const long long span = cdivll(n_tokens, S);
  if (span > 0xffffffffLL) return GLARE_ERR_UNSUPPORTED;       // a span's partial counts are 32-bit
  if (workspace_bytes < glare_vq_usage_workspace_bytes(groups, n_tokens, n_codes)) return GLARE_ERR_WORKSPACE;
  unsigned* partial = reinterpret_cast<unsigned*>(workspace);
  unsigned* oor_partial = partial + (size_t)groups * S * (size_t)n_codes;
  const int tiers = cdiv(n_codes, VU_TIER);
  hipLaunchKernelGGL(vq_usage_hist_kernel, dim3((unsigned)S, (unsigned)tiers, (unsigned)groups), dim3(VU_THREADS), 0, (hipStream_t)stream,
                     idx_i64, n_tokens, n_codes, span, partial, oor_partial);
  hipLaunchKernelGGL(vq_usage_sum_kernel, dim3((unsigned)cdiv(n_codes, VU_THREADS)), dim3(VU_THREADS), 0, (hipStream_t)stream, partial,
                     oor_partial, groups, S, n_codes, counts, out_of_range, total);
  return glare_launch_status();
}

extern "C" int glare_vq_usage_stats(const long long* counts, int rows, int n_codes, long long* tokens, long long* active, double* entropy,
                                    double* perplexity, glare_stream_t stream) {
  if (rows <= 0 || n_codes <= 0) return GLARE_ERR_INVALID;
  if (!counts || !tokens || !active || !entropy || !perplexity) return GLARE_ERR_INVALID;
  hipLaunchKernelGGL(vq_usage_stats_kernel, dim3((unsigned)rows), dim3(VU_THREADS), 0, (hipStream_t)stream, counts, n_codes, tokens, active,
                     entropy, perplexity);
  return glare_launch_status();
}
