// 4x4 convolution, padding 1, stride 1 or 2: the layers of the patch discriminator of the stage-1 GAN term (taming's
// NLayerDiscriminator: Conv2d(k = 4, s = 2 | 1, p = 1)), forward and data gradient as ONE implicit GEMM on MFMA 16x16x32; the weight
// gradient is glare_conv4x4_im2col_t_bf16 + glare_gemm_nt_bf16 (the K axis of that contraction is the pixel axis: gemm.hip).
//
//   D[n][m] = sum_{tap, c} Wp[n][tap][c] * src[pixel(m, tap)][c]
//   forward        n = Cout, c = Cin,  m = output pixel (b, oy, ox), pixel(m, tap) = (b, oy s - 1 + ky, ox s - 1 + kx)
//   data gradient  n = Cin,  c = Cout, m = input pixel (b, iy, ix),  pixel(m, tap) = (b, (iy + 1 - ky) / s, (ix + 1 - kx) / s) where s divides
// Stride-2 data gradients run as four parity classes (blockIdx.y): an input pixel of parity (py, px) meets the 2 x 2 taps with
// ky = py + 1, kx = px + 1 (mod 2) only, so each class is a dense GEMM over its four taps and no MFMA multiplies a structural zero.
//
// The filter is the MFMA's A operand (rows = n), the pixels its B operand: a lane then holds four CONSECUTIVE channels of one pixel in its
// accumulator (row = 4 (lane >> 4) + i, col = lane & 15) and stores them as one 8-byte (16-bit) or 16-byte (fp32) word.
// Both operands are read straight from global memory as 16-byte fragments (8 channels of one tap of one pixel / of one filter row): the
// crops of the training step make these launches a few hundred workgroups of a few microseconds, the filter rows of a tile are shared by
// its four waves through the L1 / L2, and there is no LDS stage whose layout could go wrong.  A source with fewer than 8 channels (the
// fp32 image of layer 1, Cin = 3; the one-channel logit gradient of layer 5) contracts over k = tap * C + c packed densely instead
// ("dense k": 48 -> 64 instead of 16 x 32), gathered element by element.
// Every sum has one order (tap-major, then channel blocks of 32, inside the MFMA its own): bitwise reproducible, no atomics.
#include "common.h"

namespace {

constexpr int C4_THREADS = 256;          // 4 waves, each 32 pixels x NT filter rows
constexpr int C4_WAVE_PIX = 32;
constexpr int C4_BLOCK_PIX = 128;

struct C4Params {
  const void* src;       // a16 or fp32 NHWC [B][SH][SW][spitch]
  const a16_t* wp;       // packed filter [Npad][16][Cp]  (dense k: [Npad][Kp])
  const float* bias;     // [N] or NULL
  void* out;             // a16 or fp32 NHWC [B][DH][DW][opitch]
  long long M;           // pixels enumerated per class
  int B, SH, SW, spitch, C, Cp;
  int DH, DW, opitch, N;
  int QH, QW;            // class grid of the stride-2 data gradient (ceil(DH / 2), ceil(DW / 2))
  int stride, dgrad, classes, dense_k, src_f32, out_f32, lrelu, vec_src, vec_out;
};

// source pixel of destination (b, y, x) under tap (ky, kx): false = padding (or, stride-2 data gradient, a tap this pixel does not meet)
__device__ __forceinline__ bool c4_src(const C4Params& p, int b, int y, int x, int ky, int kx, long long& off) {
  int sy, sx;
  if (!p.dgrad) {
    sy = y * p.stride - 1 + ky;
    sx = x * p.stride - 1 + kx;
  } else {
    sy = y + 1 - ky;
    sx = x + 1 - kx;
    if (p.stride == 2) {
      if ((sy | sx) & 1) return false;
      sy >>= 1;        // arithmetic: -2 -> -1, rejected below
      sx >>= 1;
    }
  }
  if (sy < 0 || sy >= p.SH || sx < 0 || sx >= p.SW) return false;
  off = (((long long)b * p.SH + sy) * p.SW + sx) * p.spitch;
  return true;
}

__device__ __forceinline__ float c4_load(const C4Params& p, long long idx) {
  return p.src_f32 ? static_cast<const float*>(p.src)[idx] : a2f(static_cast<const a16_t*>(p.src)[idx]);
}

template <int NF>
__global__ __launch_bounds__(C4_THREADS) void conv4x4_kernel(const C4Params p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int n0 = blockIdx.z * (16 * NF);
  const int cls = blockIdx.y, py = cls >> 1, px = cls & 1;
  const long long m0 = (long long)blockIdx.x * C4_BLOCK_PIX + wave * C4_WAVE_PIX;

  // the two pixels this lane gathers (B operand columns) -- also the pixels whose results it stores
  int pb[2], pyy[2], pxx[2];
  bool pok[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const long long m = m0 + f * 16 + lr;
    pok[f] = m < p.M;
    const long long mm = pok[f] ? m : 0;
    if (p.classes) {
      const int qx = (int)(mm % p.QW), qy = (int)((mm / p.QW) % p.QH);
      pb[f] = (int)(mm / ((long long)p.QW * p.QH));
      pyy[f] = 2 * qy + py;
      pxx[f] = 2 * qx + px;
      pok[f] = pok[f] && pyy[f] < p.DH && pxx[f] < p.DW;
    } else {
      pxx[f] = (int)(mm % p.DW);
      pyy[f] = (int)((mm / p.DW) % p.DH);
      pb[f] = (int)(mm / ((long long)p.DW * p.DH));
    }
  }

  f32x4 acc[NF][2];
#pragma unroll
  for (int i = 0; i < NF; ++i)
#pragma unroll
    for (int f = 0; f < 2; ++f) acc[i][f] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (p.dense_k) {
    // k = tap * C + c, 8 consecutive k per lane and 32 per MFMA; the packed filter row is [Kp]
    const int K = 16 * p.C, Kp = p.Cp;
    for (int k0 = 0; k0 < Kp; k0 += 32) {
      const int kb = k0 + 8 * lk;
      a16x8 bf[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = kb + j;
          float e = 0.f;
          if (pok[f] && k < K) {
            const int tap = k / p.C, c = k - tap * p.C;
            long long off;
            if (c4_src(p, pb[f], pyy[f], pxx[f], tap >> 2, tap & 3, off)) e = c4_load(p, off + c);
          }
          v[j >> 1] |= (uint32_t)f2a(e) << (16 * (j & 1));
        }
        bf[f] = __builtin_bit_cast(a16x8, v);
      }
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        const a16x8 af = __builtin_bit_cast(a16x8, *reinterpret_cast<const u32x4*>(p.wp + (long long)(n0 + i * 16 + lr) * Kp + kb));
#pragma unroll
        for (int f = 0; f < 2; ++f) acc[i][f] = mfma_a16_16x16x32(af, bf[f], acc[i][f], 0, 0, 0);
      }
    }
  } else {
    const int ntaps = p.classes ? 4 : 16;
    const int ky0 = (py + 1) & 1, kx0 = (px + 1) & 1;
    for (int t = 0; t < ntaps; ++t) {
      const int ky = p.classes ? ky0 + 2 * (t >> 1) : t >> 2, kx = p.classes ? kx0 + 2 * (t & 1) : t & 3;
      const int tap = ky * 4 + kx;
      long long soff[2] = {0, 0};
      bool sok[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) sok[f] = pok[f] && c4_src(p, pb[f], pyy[f], pxx[f], ky, kx, soff[f]);
      const a16_t* wt = p.wp + ((long long)(n0 + lr) * 16 + tap) * p.Cp + 8 * lk;
      for (int c0 = 0; c0 < p.Cp; c0 += 32) {
        const int c = c0 + 8 * lk;
        a16x8 bf[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          u32x4 v = {0u, 0u, 0u, 0u};
          if (sok[f] && c < p.C) {
            if (p.vec_src && c + 8 <= p.C) {
              v = *reinterpret_cast<const u32x4*>(static_cast<const a16_t*>(p.src) + soff[f] + c);
            } else {
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const float e = (c + j < p.C) ? c4_load(p, soff[f] + c + j) : 0.f;
                v[j >> 1] |= (uint32_t)f2a(e) << (16 * (j & 1));
              }
            }
          }
          bf[f] = __builtin_bit_cast(a16x8, v);
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
          const a16x8 af = __builtin_bit_cast(a16x8, *reinterpret_cast<const u32x4*>(wt + (long long)i * 16 * 16 * p.Cp + c0));
#pragma unroll
          for (int f = 0; f < 2; ++f) acc[i][f] = mfma_a16_16x16x32(af, bf[f], acc[i][f], 0, 0, 0);
        }
      }
    }
  }

  // epilogue: lane = pixel (lane & 15) of each fragment, rows n = n0 + 16 i + 4 (lane >> 4) + 0..3
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    if (!pok[f]) continue;
    const long long dpix = ((long long)pb[f] * p.DH + pyy[f]) * p.DW + pxx[f];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const int n = n0 + i * 16 + 4 * lk;
      if (n >= p.N) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float a = acc[i][f][r];
        if (p.bias && n + r < p.N) a += p.bias[n + r];
        if (p.lrelu) a = a > 0.f ? a : 0.2f * a;
        v[r] = a;
      }
      const long long o = dpix * p.opitch + n;
      if (p.vec_out && n + 4 <= p.N) {
        if (p.out_f32) {
          *reinterpret_cast<f32x4*>(static_cast<float*>(p.out) + o) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
          *reinterpret_cast<u32x2*>(static_cast<a16_t*>(p.out) + o) = u32x2{pack_a2(v[0], v[1]), pack_a2(v[2], v[3])};
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < p.N) {
            if (p.out_f32) static_cast<float*>(p.out)[o + r] = v[r];
            else static_cast<a16_t*>(p.out)[o + r] = f2a(v[r]);
          }
      }
    }
  }
}

// packed[n][tap][c] (dense k: packed[n][tap * C + c]) from the fp32 OIHW filter; rows n >= N and channels c >= C zero
__global__ __launch_bounds__(256) void conv4x4_pack_kernel(const float* __restrict__ w, int Co, int Ci, int dgrad, int dense_k, int N, int C,
                                                           int Cp, long long total, a16_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  int n, tap, c;
  if (dense_k) {
    n = (int)(i / Cp);
    const int k = (int)(i % Cp);
    tap = k / C;
    c = k - tap * C;
    if (k >= 16 * C) n = N;   // the tail of the row: zero
  } else {
    c = (int)(i % Cp);
    tap = (int)((i / Cp) % 16);
    n = (int)(i / ((long long)Cp * 16));
  }
  float v = 0.f;
  if (n < N && c < C) {
    const int co = dgrad ? c : n, ci = dgrad ? n : c;
    v = w[((long long)co * Ci + ci) * 16 + tap];
  }
  out[i] = f2a(v);
}

// colT[ci * 16 + tap][p] = x[b, oy s - 1 + ky, ox s - 1 + kx, ci] (0 in the padding), p = (b, oy, ox); columns [P, ldp) zero;
// row 16 Ci = ones for p < P (the bias gradient's operand).  x: a16 or fp32 NHWC.
__global__ __launch_bounds__(256) void conv4x4_im2col_t_kernel(const void* __restrict__ x, int x_f32, int H, int W, int pitch, int Ci,
                                                               int stride, int OH, int OW, long long P, a16_t* __restrict__ col,
                                                               long long ldp, int ones_row) {
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  const int row = blockIdx.y;
  if (pix >= ldp) return;
  if (row == Ci * 16) {
    if (ones_row >= 0) col[(long long)ones_row * ldp + pix] = pix < P ? (a16_t)A16_ONE : (a16_t)0;
    return;
  }
  const int c = row >> 4, tap = row & 15, ky = tap >> 2, kx = tap & 3;
  a16_t v = 0;
  if (pix < P) {
    const int ox = (int)(pix % OW), oy = (int)((pix / OW) % OH), b = (int)(pix / ((long long)OW * OH));
    const int iy = oy * stride - 1 + ky, ix = ox * stride - 1 + kx;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
      const long long idx = (((long long)b * H + iy) * W + ix) * pitch + c;
      v = x_f32 ? f2a(static_cast<const float*>(x)[idx]) : static_cast<const a16_t*>(x)[idx];
    }
  }
  col[(long long)row * ldp + pix] = v;
}

inline int c4_out(int in, int stride) { return (in + 2 - 4) / stride + 1; }
inline int c4_nt(int N) { return N <= 16 ? 16 : 64; }
inline bool c4_dense(int C) { return C < 8; }
inline int rup(int a, int b) { return (a + b - 1) / b * b; }

}  // namespace

extern "C" long long glare_conv4x4_packed_elems(int Cout, int Cin, int dgrad) {
  if (Cout <= 0 || Cin <= 0) return 0;
  const int N = dgrad ? Cin : Cout, C = dgrad ? Cout : Cin;
  const long long npad = rup(N, c4_nt(N));
  return c4_dense(C) ? npad * rup(16 * C, 32) : npad * 16 * rup(C, 32);
}

extern "C" int glare_conv4x4_pack_bf16(const float* w_oihw, int Cout, int Cin, int dgrad, void* packed, glare_stream_t stream) {
  if (!w_oihw || !packed || Cout <= 0 || Cin <= 0) return GLARE_ERR_INVALID;
  const int N = dgrad ? Cin : Cout, C = dgrad ? Cout : Cin;
  const int dense = c4_dense(C) ? 1 : 0;
  const int Cp = dense ? rup(16 * C, 32) : rup(C, 32);
  const long long total = glare_conv4x4_packed_elems(Cout, Cin, dgrad);
  if (cdivll(total, 256) > 0x7fffffffLL) return GLARE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(conv4x4_pack_kernel, dim3((unsigned)cdivll(total, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w_oihw, Cout, Cin,
                     dgrad ? 1 : 0, dense, N, C, Cp, total, static_cast<a16_t*>(packed));
  return glare_launch_status();
}

static int c4_launch(C4Params& p, int Cout, int Cin, glare_stream_t stream) {
  p.dense_k = c4_dense(p.C) ? 1 : 0;
  p.Cp = p.dense_k ? rup(16 * p.C, 32) : rup(p.C, 32);
  p.classes = (p.dgrad && p.stride == 2 && !p.dense_k) ? 1 : 0;
  p.QH = (p.DH + 1) / 2;
  p.QW = (p.DW + 1) / 2;
  p.M = p.classes ? (long long)p.B * p.QH * p.QW : (long long)p.B * p.DH * p.DW;
  // 16-byte operand reads / 8- and 16-byte stores need the alignment; everything else goes element by element
  p.vec_src = (!p.src_f32 && p.spitch % 8 == 0 && (reinterpret_cast<uintptr_t>(p.src) & 15) == 0) ? 1 : 0;
  p.vec_out = (p.opitch % 4 == 0 && (reinterpret_cast<uintptr_t>(p.out) & 15) == 0) ? 1 : 0;
  const long long blocks = cdivll(p.M, C4_BLOCK_PIX);
  if (blocks > 0x7fffffffLL) return GLARE_ERR_UNSUPPORTED;
  const int nt = c4_nt(p.N);
  const int nz = cdiv(p.N, nt);
  if (nz > 65535) return GLARE_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks, p.classes ? 4 : 1, (unsigned)nz);
  if (nt == 16)
    hipLaunchKernelGGL(conv4x4_kernel<1>, grid, dim3(C4_THREADS), 0, static_cast<hipStream_t>(stream), p);
  else
    hipLaunchKernelGGL(conv4x4_kernel<4>, grid, dim3(C4_THREADS), 0, static_cast<hipStream_t>(stream), p);
  return glare_launch_status();
}

extern "C" int glare_conv4x4_forward_bf16(const void* x, int x_is_f32, int x_pitch, const void* packed, const float* bias, void* y,
                                          int y_is_f32, int y_pitch, int B, int H, int W, int Cin, int Cout, int stride, int lrelu,
                                          glare_stream_t stream) {
  if (!x || !packed || !y || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return GLARE_ERR_INVALID;
  if (stride != 1 && stride != 2) return GLARE_ERR_INVALID;
  if (x_pitch < Cin || y_pitch < Cout) return GLARE_ERR_INVALID;
  const int OH = c4_out(H, stride), OW = c4_out(W, stride);
  if (H + 2 < 4 || W + 2 < 4 || OH <= 0 || OW <= 0) return GLARE_ERR_INVALID;
  // pixel indices are 32-bit in the kernel's decode (element offsets are 64-bit)
  if ((long long)B * H * W >= (1ll << 31) || (long long)B * OH * OW >= (1ll << 31)) return GLARE_ERR_UNSUPPORTED;
  C4Params p;
  p.src = x; p.wp = static_cast<const a16_t*>(packed); p.bias = bias; p.out = y;
  p.B = B; p.SH = H; p.SW = W; p.spitch = x_pitch; p.C = Cin;
  p.DH = OH; p.DW = OW; p.opitch = y_pitch; p.N = Cout;
  p.stride = stride; p.dgrad = 0; p.src_f32 = x_is_f32 ? 1 : 0; p.out_f32 = y_is_f32 ? 1 : 0; p.lrelu = lrelu ? 1 : 0;
  return c4_launch(p, Cout, Cin, stream);
}

extern "C" int glare_conv4x4_dgrad_bf16(const void* g, int g_pitch, const void* packed, void* dx, int dx_is_f32, int dx_pitch, int B, int H,
                                        int W, int Cin, int Cout, int stride, glare_stream_t stream) {
  if (!g || !packed || !dx || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return GLARE_ERR_INVALID;
  if (stride != 1 && stride != 2) return GLARE_ERR_INVALID;
  if (g_pitch < Cout || dx_pitch < Cin) return GLARE_ERR_INVALID;
  const int OH = c4_out(H, stride), OW = c4_out(W, stride);
  if (H + 2 < 4 || W + 2 < 4 || OH <= 0 || OW <= 0) return GLARE_ERR_INVALID;
  if ((long long)B * H * W >= (1ll << 31) || (long long)B * OH * OW >= (1ll << 31)) return GLARE_ERR_UNSUPPORTED;
  C4Params p;
  p.src = g; p.wp = static_cast<const a16_t*>(packed); p.bias = nullptr; p.out = dx;
  p.B = B; p.SH = OH; p.SW = OW; p.spitch = g_pitch; p.C = Cout;
  p.DH = H; p.DW = W; p.opitch = dx_pitch; p.N = Cin;
  p.stride = stride; p.dgrad = 1; p.src_f32 = 0; p.out_f32 = dx_is_f32 ? 1 : 0; p.lrelu = 0;
  return c4_launch(p, Cout, Cin, stream);
}

extern "C" int glare_conv4x4_im2col_t_bf16(const void* x, int x_is_f32, int x_pitch, int B, int H, int W, int Cin, int stride, void* colT,
                                           long long ldp, int ones_row, glare_stream_t stream) {
  if (!x || !colT || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || x_pitch < Cin) return GLARE_ERR_INVALID;
  if (stride != 1 && stride != 2) return GLARE_ERR_INVALID;
  const int OH = c4_out(H, stride), OW = c4_out(W, stride);
  if (H + 2 < 4 || W + 2 < 4 || OH <= 0 || OW <= 0) return GLARE_ERR_INVALID;
  const long long P = (long long)B * OH * OW;
  if (ldp < P || ldp % 64 != 0) return GLARE_ERR_INVALID;
  if ((long long)B * H * W >= (1ll << 31) || P >= (1ll << 31)) return GLARE_ERR_UNSUPPORTED;
  if (ones_row >= 0 && ones_row != Cin * 16) return GLARE_ERR_INVALID;
  const long long rows = (long long)Cin * 16 + (ones_row >= 0 ? 1 : 0);
  if (rows > 65535) return GLARE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(conv4x4_im2col_t_kernel, dim3((unsigned)cdivll(ldp, 256), (unsigned)rows), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                     x_is_f32 ? 1 : 0, H, W, x_pitch, Cin, stride, OH, OW, P, static_cast<a16_t*>(colT), ldp, ones_row);
  return glare_launch_status();
}
