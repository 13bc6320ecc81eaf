// One training batch from a device-resident uint8 dataset (training side): what LoL_Dataset.__getitem__
// (code/data/LoL_dataset.py:409-502) does per sample on the host -- random_crop (:640-661), np.flip(axis = 1) (:615-621),
// np.rot90(k, axes = (0, 1)) (:631-637), ToTensor's /255, log(clamp(x + 1e-3, min = 1e-3)) on the low image -- as ONE launch for
// the whole batch, written straight into the fp32 NCHW buffers the training step reads.  The random decisions stay on the host
// (glare_amd.data.draw_augmentation: the reference's np.random call order); they arrive as one int32 row per sample.
// HBM- and launch-bound and tiny (stage 2, 4 x 320^2: 2.4 MB read, 9.8 MB written): one thread per output pixel, no tuning.
#include "common.h"

namespace {

constexpr int R = GLARE_TRAIN_ROW_INTS;   // { offset lo, offset hi, H, W, y0, x0, crop_h, crop_w, flip, k }

__global__ __launch_bounds__(256) void train_batch_kernel(const uint8_t* __restrict__ low, const uint8_t* __restrict__ high, long long n_bytes,
                                                          const int* __restrict__ rows, int B, int OH, int OW,
                                                          const float* __restrict__ lut, float* __restrict__ gt, float* __restrict__ lq) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long plane = (long long)OH * OW;
  if (i >= (long long)B * plane) return;
  const int b = (int)(i / plane);
  const long long p = i - (long long)b * plane;
  const int oy = (int)(p / OW), ox = (int)(p - (long long)oy * OW);
  const int* row = rows + (long long)b * R;
  const long long off = (long long)(uint32_t)row[0] | ((long long)row[1] << 32);
  const int H = row[2], W = row[3], y0 = row[4], x0 = row[5], ch = row[6], cw = row[7], flip = row[8], k = row[9];
  // out = rot90(F, k) with F = flip(crop):  k = 1: out[i][j] = F[j][cw - 1 - i];  k = 3: out[i][j] = F[ch - 1 - j][i]
  int r = oy, c = ox;
  if (k == 1) { r = ox; c = cw - 1 - oy; }
  if (k == 3) { r = ch - 1 - ox; c = oy; }
  if (flip) c = cw - 1 - c;
  const int ys = y0 + r, xs = x0 + c;
  // the host entry has validated the rows it was given; a replayed launch reads rows it never saw: never dereference outside
  if (ys < 0 || ys >= H || xs < 0 || xs >= W || off < 0 || off + 3LL * H * W > n_bytes) return;
  const long long src = off + ((long long)ys * W + xs) * 3;
  float* g = gt + (long long)b * 3 * plane + p;
  float* l = lq + (long long)b * 3 * plane + p;
#pragma unroll
  for (int ch3 = 0; ch3 < 3; ++ch3) {
    g[ch3 * plane] = __fdiv_rn((float)high[src + ch3], 255.f);      // .float().div(255): IEEE division
    l[ch3 * plane] = lut[low[src + ch3]];
  }
}

}  // namespace

extern "C" int glare_train_batch_u8(const unsigned char* low_u8, const unsigned char* high_u8, long long n_bytes, const int* rows_host,
                                    const int* rows_device, int B, int out_h, int out_w, const float* lq_lut_256, float* gt_nchw,
                                    float* lq_nchw, glare_stream_t stream) {
  if (!low_u8 || !high_u8 || !rows_host || !rows_device || !lq_lut_256 || !gt_nchw || !lq_nchw) return GLARE_ERR_INVALID;
  if (B <= 0 || out_h <= 0 || out_w <= 0 || n_bytes <= 0) return GLARE_ERR_INVALID;
  for (int b = 0; b < B; ++b) {
    const int* row = rows_host + (size_t)b * R;
    const long long off = (long long)(uint32_t)row[0] | ((long long)row[1] << 32);
    const int H = row[2], W = row[3], y0 = row[4], x0 = row[5], ch = row[6], cw = row[7], flip = row[8], k = row[9];
    if (H <= 0 || W <= 0 || off < 0 || off + 3LL * H * W > n_bytes) return GLARE_ERR_INVALID;
    if (y0 < 0 || x0 < 0 || ch <= 0 || cw <= 0 || (long long)y0 + ch > H || (long long)x0 + cw > W) return GLARE_ERR_INVALID;
    if ((flip != 0 && flip != 1) || (k != 0 && k != 1 && k != 3)) return GLARE_ERR_INVALID;
    if (k != 0 && ch != cw) return GLARE_ERR_INVALID;
    if (ch != out_h || cw != out_w) return GLARE_ERR_INVALID;      // with k != 0 the crop is square: one test covers both
  }
  const long long blocks = cdivll((long long)B * out_h * out_w, 256);
  if (blocks > 0x7fffffffLL) return GLARE_ERR_INVALID;
  hipLaunchKernelGGL(train_batch_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), low_u8, high_u8, n_bytes,
                     rows_device, B, out_h, out_w, lq_lut_256, gt_nchw, lq_nchw);
  return glare_launch_status();
}
