// Codebook restart: the codes a window's histogram shows nothing selected are re-seeded from the current batch's latents.
//
// dE of csrc/vq_train.hip is exactly 0 for a code no token selected, so such a code never moves.  glare_vq_restart_f32 (semantics:
// include/glare_hip.h) ranks the dead codes d_0 < d_1 < ... and copies token t_j = (offset + j * stride) mod N into row d_j, j < R =
// min(D, N), stride = N / R, clearing the row's Adam moments.  D, R and stride never leave the device.  Four launches:
//   count   one code per thread: dead = window[k] <= threshold; a wave64 ballot + popcount per wave, the four wave totals through LDS,
//           one total per workgroup (a plain store)
//   scan    ONE workgroup: the exclusive scan of the <= 4096 workgroup totals (a thread adds its run of consecutive totals, a fixed
//           Hillis-Steele scan of the 256 run sums in LDS), and the header {D, R, stride, offset mod N}; n_dead[0] = D
//   apply   the ballot again: rank j = workgroup offset + the waves in front + the dead lanes below; j < R and a finite source: the row
//           and its moments are written; window[k] = 0; the workgroup's count of written rows (ballot + popcount again)
//   finish  ONE workgroup adds the per-workgroup counts in a fixed order: n_restarted[0]
// Integers only, so every sum is exact and the same on every run; no atomics of any kind.  The data-dependent addresses: z[t], t an
// UNSIGNED remainder of N whatever the header holds, and row k behind k < K -- the scan's loop index, not a loaded value.
// glare_vq_restart_ema_f32: the same launches for an EMA codebook -- a written row is also its embed_avg row, cluster_size[k] = seed_size.
// Rows are copied as 32-bit words: a bit copy.  Compiled with -ffp-contract=off like the other vq*.hip (no float arithmetic here at all).
#include "common.h"

namespace {

constexpr int VR_THREADS = 256;
constexpr int VR_WAVES = VR_THREADS / GLARE_WAVE;
constexpr int VR_HEADER = 4;                          // long long cells in front of the workspace: D, R, stride, offset mod N

struct DeadRank {
  bool dead;
  unsigned in_group;                                  // dead codes of this workgroup in front of this one
};

// Levels 1 and 2 of the scan, for code k of this workgroup.  Every thread of the workgroup calls it (a ballot and two barriers).
__device__ __forceinline__ DeadRank dead_rank(const long long* __restrict__ window, long long threshold, int k, int K, unsigned* wave_tot,
                                              unsigned* group_tot) {
  const bool dead = k < K && window[k] <= threshold;
  const unsigned long long mask = __ballot(dead);    // 64 bits on gfx950
  const int lane = threadIdx.x & (GLARE_WAVE - 1), wave = threadIdx.x / GLARE_WAVE;
  const unsigned below = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
  __syncthreads();                                    // (a second call reuses wave_tot)
  if (lane == 0) wave_tot[wave] = (unsigned)__popcll(mask);
  __syncthreads();
  unsigned front = 0u, all = 0u;
#pragma unroll
  for (int w = 0; w < VR_WAVES; ++w) {
    front += w < wave ? wave_tot[w] : 0u;
    all += wave_tot[w];
  }
  *group_tot = all;
  return DeadRank{dead, front + below};
}

__global__ __launch_bounds__(VR_THREADS) void vq_restart_count_kernel(const long long* __restrict__ window, long long threshold, int K,
                                                                      unsigned* __restrict__ group_dead) {
  __shared__ unsigned wave_tot[VR_WAVES];
  unsigned total;
  dead_rank(window, threshold, (int)(blockIdx.x * VR_THREADS + threadIdx.x), K, wave_tot, &total);
  if (threadIdx.x == 0) group_dead[blockIdx.x] = total;
}

__global__ __launch_bounds__(VR_THREADS) void vq_restart_scan_kernel(const unsigned* __restrict__ group_dead, int groups, long long N,
                                                                     long long offset, unsigned* __restrict__ group_off,
                                                                     long long* __restrict__ header, long long* __restrict__ n_dead) {
  __shared__ unsigned run[VR_THREADS];
  const int per = (groups + VR_THREADS - 1) / VR_THREADS;
  const int g0 = (int)threadIdx.x * per, g1 = g0 + per < groups ? g0 + per : groups;
  unsigned mine = 0u;
  for (int g = g0; g < g1; ++g) mine += group_dead[g];
  run[threadIdx.x] = mine;
  __syncthreads();
  for (int o = 1; o < VR_THREADS; o <<= 1) {          // inclusive scan of the run sums, a fixed tree
    const unsigned add = (int)threadIdx.x >= o ? run[threadIdx.x - o] : 0u;
    __syncthreads();
    run[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned at = run[threadIdx.x] - mine;
  for (int g = g0; g < g1; ++g) {
    group_off[g] = at;
    at += group_dead[g];
  }
  if (threadIdx.x == 0) {
    const long long D = (long long)run[VR_THREADS - 1];
    const long long R = D < N ? D : N;
    header[0] = D;
    header[1] = R;
    header[2] = R > 0 ? N / R : 0;
    header[3] = ((offset % N) + N) % N;
    n_dead[0] = D;
  }
}

__global__ __launch_bounds__(VR_THREADS) void vq_restart_apply_kernel(long long* __restrict__ window, long long threshold,
                                                                      const uint32_t* __restrict__ z, long long N, int K,
                                                                      const unsigned* __restrict__ group_off,
                                                                      const long long* __restrict__ header, uint32_t* __restrict__ codebook,
                                                                      uint32_t* __restrict__ exp_avg, uint32_t* __restrict__ exp_avg_sq,
                                                                      uint32_t* __restrict__ embed_avg, float* __restrict__ cluster_size,
                                                                      float seed_size, unsigned* __restrict__ group_written) {
  __shared__ unsigned wave_tot[VR_WAVES];
  const int k = (int)(blockIdx.x * VR_THREADS + threadIdx.x);
  unsigned total;
  const DeadRank r = dead_rank(window, threshold, k, K, wave_tot, &total);
  const long long R = header[1], stride = header[2], off = header[3];
  const long long j = (long long)group_off[blockIdx.x] + (long long)r.in_group;
  bool wrote = false;
  if (r.dead && j < R) {
    // j * stride <= R * stride <= N and off < N; the remainder is unsigned, so t < N for any header
    const size_t t = (size_t)((unsigned long long)(off + j * stride) % (unsigned long long)N);
    const uint32_t a = z[3 * t], b = z[3 * t + 1], c = z[3 * t + 2];
    const uint32_t EXP = 0x7f800000u;                 // an exponent of all ones: inf or NaN
    if ((a & EXP) != EXP && (b & EXP) != EXP && (c & EXP) != EXP) {
      const size_t row = 3 * (size_t)k;
      codebook[row] = a;
      codebook[row + 1] = b;
      codebook[row + 2] = c;
      if (exp_avg) {
        exp_avg[row] = exp_avg[row + 1] = exp_avg[row + 2] = 0u;
        exp_avg_sq[row] = exp_avg_sq[row + 1] = exp_avg_sq[row + 2] = 0u;
      }
      if (embed_avg) {                                // the EMA form: the running sum restarts at the row, its weight at seed_size
        embed_avg[row] = a;
        embed_avg[row + 1] = b;
        embed_avg[row + 2] = c;
        cluster_size[k] = seed_size;
      }
      wrote = true;
    }
  }
  if (k < K) window[k] = 0;
  const unsigned long long mask = __ballot(wrote);
  __syncthreads();                                    // every read of wave_tot in dead_rank is behind us
  if ((threadIdx.x & (GLARE_WAVE - 1)) == 0) wave_tot[threadIdx.x / GLARE_WAVE] = (unsigned)__popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned w = 0u;
#pragma unroll
    for (int i = 0; i < VR_WAVES; ++i) w += wave_tot[i];
    group_written[blockIdx.x] = w;
  }
}

__global__ __launch_bounds__(VR_THREADS) void vq_restart_finish_kernel(const unsigned* __restrict__ group_written, int groups,
                                                                       long long* __restrict__ n_restarted) {
  __shared__ long long red[VR_THREADS];
  long long s = 0;
  for (int g = threadIdx.x; g < groups; g += VR_THREADS) s += (long long)group_written[g];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = VR_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) n_restarted[0] = red[0];
}

}  // namespace

extern "C" size_t glare_vq_restart_workspace_bytes(int n_codes) {
  if (n_codes <= 0 || n_codes > GLARE_VQ_USAGE_MAX_CODES) return 0;
  // [D, R, stride, offset] int64, then per workgroup: its dead codes, their exclusive scan, the rows it wrote
  return VR_HEADER * sizeof(long long) + 3 * (size_t)cdiv(n_codes, VR_THREADS) * sizeof(unsigned);
}

namespace {

// Both entries: the same four launches; embed_avg / cluster_size are the EMA form's, exp_avg / exp_avg_sq the gradient form's.
int restart_launch(long long* window_counts, long long threshold, const float* z_tokens, long long n_tokens, int n_codes, int dim,
                   long long offset, float* codebook, float* exp_avg, float* exp_avg_sq, float* embed_avg, float* cluster_size,
                   float seed_size, long long* n_dead, long long* n_restarted, void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  if (((uintptr_t)workspace & 7u) != 0) return GLARE_ERR_INVALID;
  if (dim != 3 || n_codes > GLARE_VQ_USAGE_MAX_CODES) return GLARE_ERR_UNSUPPORTED;
  if (workspace_bytes < glare_vq_restart_workspace_bytes(n_codes)) return GLARE_ERR_WORKSPACE;
  const int groups = cdiv(n_codes, VR_THREADS);
  long long* header = reinterpret_cast<long long*>(workspace);
  unsigned* group_dead = reinterpret_cast<unsigned*>(header + VR_HEADER);
  unsigned* group_off = group_dead + groups;
  unsigned* group_written = group_off + groups;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(vq_restart_count_kernel, dim3((unsigned)groups), dim3(VR_THREADS), 0, s, window_counts, threshold, n_codes, group_dead);
  hipLaunchKernelGGL(vq_restart_scan_kernel, dim3(1), dim3(VR_THREADS), 0, s, group_dead, groups, n_tokens, offset, group_off, header, n_dead);
  hipLaunchKernelGGL(vq_restart_apply_kernel, dim3((unsigned)groups), dim3(VR_THREADS), 0, s, window_counts, threshold,
                     reinterpret_cast<const uint32_t*>(z_tokens), n_tokens, n_codes, group_off, header, reinterpret_cast<uint32_t*>(codebook),
                     reinterpret_cast<uint32_t*>(exp_avg), reinterpret_cast<uint32_t*>(exp_avg_sq), reinterpret_cast<uint32_t*>(embed_avg),
                     cluster_size, seed_size, group_written);
  hipLaunchKernelGGL(vq_restart_finish_kernel, dim3(1), dim3(VR_THREADS), 0, s, group_written, groups, n_restarted);
  return glare_launch_status();
}

}  // namespace

extern "C" int glare_vq_restart_f32(long long* window_counts, long long threshold, const float* z_tokens, long long n_tokens, int n_codes,
                                    int dim, long long offset, float* codebook, float* exp_avg, float* exp_avg_sq, long long* n_dead,
                                    long long* n_restarted, void* workspace, size_t workspace_bytes, glare_stream_t stream) {
  if (n_tokens <= 0 || n_codes <= 0 || dim <= 0) return GLARE_ERR_INVALID;
  if (!window_counts || !z_tokens || !codebook || !n_dead || !n_restarted || !workspace) return GLARE_ERR_INVALID;
  if ((exp_avg == nullptr) != (exp_avg_sq == nullptr)) return GLARE_ERR_INVALID;
  return restart_launch(window_counts, threshold, z_tokens, n_tokens, n_codes, dim, offset, codebook, exp_avg, exp_avg_sq, nullptr, nullptr,
                        0.f, n_dead, n_restarted, workspace, workspace_bytes, stream);
}

// The restart under an EMA codebook (csrc/vq_ema.hip): the same dead codes, ranking and source tokens; a written row also becomes its
// embed_avg row (a bit copy) and cluster_size[k] = seed_size.  No Adam moments: the codebook is no Adam parameter there.
extern "C" int glare_vq_restart_ema_f32(long long* window_counts, long long threshold, const float* z_tokens, long long n_tokens, int n_codes,
                                        int dim, long long offset, float seed_size, float* codebook, float* embed_avg, float* cluster_size,
                                        long long* n_dead, long long* n_restarted, void* workspace, size_t workspace_bytes,
                                        glare_stream_t stream) {
  if (n_tokens <= 0 || n_codes <= 0 || dim <= 0) return GLARE_ERR_INVALID;
  if (!window_counts || !z_tokens || !codebook || !embed_avg || !cluster_size || !n_dead || !n_restarted || !workspace) return GLARE_ERR_INVALID;
  if (!(seed_size >= 0.f && seed_size <= 3.0e38f)) return GLARE_ERR_INVALID;       // finite and not negative (a NaN fails both)
  return restart_launch(window_counts, threshold, z_tokens, n_tokens, n_codes, dim, offset, codebook, nullptr, nullptr, embed_avg,
                        cluster_size, seed_size, n_dead, n_restarted, workspace, workspace_bytes, stream);
}
