"""The data movers and the NT GEMM behind the GEMM-form weight gradients restated in plain torch: the references of
test_gpu_helper_kernels.py.  Each is written from the contract in include/glare_hip.h and the header comments of csrc/gemm.hip and
csrc/train_ops.hip (what lands where), with explicit index arithmetic, and test_helpers_fp64_host.py checks every one against
F.unfold and fp64 AUTOGRAD of the forward operation -- so that the GPU test's reference is not a copy of the code under test.
reduce_parts_f32 is the one restatement in fp32: it replays the documented ORDER of the two reduction kernels, so that its bit pattern
is what the kernel must produce.  The second half holds what both test files share: the sentinel buffers and the bit-for-bit
comparison of the data movers (the host test checks that the comparison sees a swapped row, a one-ulp tail column and a one-ulp
element), and the exact-arithmetic operands of the GEMM with the condition that makes them worth running.  A plain module like
tolerances.py; nothing here touches the library."""
import torch

# ---- restatements ------------------------------------------------------------------------------------------------------------------


def conv_out_size(size, ksize, stride, pad):
    """stride 1: size + 2 pad - k + 1; stride 2: the (0,1,0,1) padding of Downsample, (size + 1 - k) // 2 + 1"""
    return max(0, (size + 1 - ksize) // 2 + 1 if stride == 2 else size + 2 * pad - ksize + 1)


def im2col_t(x_nhwc, ksize, stride, pad, upsample):
    """x [B, H, W, Ci] -> [Ci k k, P]: row c k k + ty k + tx, column p = (b OH + oy) OW + ox holds x[b, oy s + ty - pad, ox s + tx - pad, c]
    of the (nearest x2 upsampled) image, 0 outside it.  Stride 2 pads on the far side only (pad = 0 here, one row / column beyond)."""
    B, H, W, Ci = x_nhwc.shape
    IH, IW = (2 * H, 2 * W) if upsample else (H, W)
    OH, OW = conv_out_size(IH, ksize, stride, pad), conv_out_size(IW, ksize, stride, pad)
    out = torch.zeros(Ci, ksize * ksize, B, OH, OW, dtype=x_nhwc.dtype, device=x_nhwc.device)
    oy, ox = torch.arange(OH, device=x_nhwc.device), torch.arange(OW, device=x_nhwc.device)
    for ty in range(ksize):
        for tx in range(ksize):
            iy, ix = oy * stride + ty - pad, ox * stride + tx - pad
            oky, okx = (iy >= 0) & (iy < IH), (ix >= 0) & (ix < IW)
            sy, sx = (iy // 2 if upsample else iy)[oky], (ix // 2 if upsample else ix)[okx]
            if sy.numel() == 0 or sx.numel() == 0:
                continue
            v = x_nhwc[:, sy][:, :, sx]                                     # [B, oy', ox', Ci]
            dst = out[:, ty * ksize + tx]                                   # [Ci, B, OH, OW]
            dst[:, :, oky.nonzero()[:, 0, None], okx.nonzero()[None, :, 0]] = v.permute(3, 0, 1, 2)
    return out.reshape(Ci * ksize * ksize, B * OH * OW)


def dilate2(g):
    """[B, OH, OW, C] -> [B, 2 OH, 2 OW, C]: out[b, 2 oy + 1, 2 ox + 1] = g[b, oy, ox], 0 elsewhere"""
    B, OH, OW, C = g.shape
    pick = torch.zeros(2, dtype=g.dtype, device=g.device)
    pick[1] = 1.0
    out = torch.einsum("bhwc,i,j->bhiwjc", g, pick, pick).reshape(B, 2 * OH, 2 * OW, C)
    hole = torch.ones(2 * OH, 2 * OW, dtype=torch.bool, device=g.device)
    hole[1::2, 1::2] = False
    out[:, hole] = 0.0          # +0: a negative value times the 0 of `pick` is -0, and the contract is zero BITS
    return out


def pool2_sum(g):
    """[B, 2 H, 2 W, C] -> [B, H, W, C]: the sum of every 2 x 2 block"""
    B, H2, W2, C = g.shape
    assert H2 % 2 == 0 and W2 % 2 == 0
    return torch.einsum("bhiwjc->bhwc", g.reshape(B, H2 // 2, 2, W2 // 2, 2, C))


def colsum(g2d):
    return torch.einsum("pc->c", g2d)


def transpose_padded(x, ld_out):
    """[.., R, C] -> [.., C, ld_out]: out[c, r] = x[r, c], columns [R, ld_out) zero"""
    R = x.shape[-2]
    t = torch.einsum("...rc->...cr", x)
    return torch.cat([t, torch.zeros(*t.shape[:-1], ld_out - R, dtype=x.dtype, device=x.device)], -1)          # +0 bits


def gemm_nt(a, b, alpha=1.0):
    """alpha sum_k a[.., m, k] b[.., n, k]"""
    return alpha * torch.einsum("...mk,...nk->...mn", a, b)


def many_parts(n_parts, n):
    """glare_reduce_parts_grouped_f32's choice of kernel (csrc/gemm.hip)"""
    return n_parts >= 32 and n <= 65536


def reduce_parts_f32(parts32, scale, n, old=None):
    """parts32 fp32 [S, n] on the CPU -> fp32 [n], in the kernels' order: one ascending chain from 0, or (many_parts) 16 chains of the
    parts s = j (mod 16), each ascending from 0, joined in order j = 0..15; then * scale, then old + (accumulating)."""
    assert parts32.dtype == torch.float32 and parts32.device.type == "cpu" and parts32.shape[1] == n
    S = parts32.shape[0]
    f32 = torch.float32

    def chain(rows):
        s = torch.zeros(n, dtype=f32)
        for k in rows:
            s = torch.add(s, parts32[k])
        return s

    if many_parts(S, n):
        s = chain(range(0, S, 16))
        for j in range(1, 16):
            s = torch.add(s, chain(range(j, S, 16)))
    else:
        s = chain(range(S))
    s = torch.mul(s, torch.tensor(scale, dtype=f32))
    return s if old is None else torch.add(old.to(f32), s)


def colsum_blocks(P):
    """glare_colsum_bf16's split of the pixel axis -> (blocks, pixels per block)"""
    blocks = min(max(-(-P // 512), 1), 256)
    return blocks, -(-P // blocks)


# ---- sentinel buffers and the comparison of the data movers -------------------------------------------------------------------------
SENTINEL16 = 0x7B7B          # int16 pattern of every 16-bit element a kernel must not write (test_gpu_attn_schedule.py)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def sentinel16(shape, dtype, device="cpu"):
    return torch.full(tuple(shape), SENTINEL16, dtype=torch.int16, device=device).view(dtype)


def rounded_exactly(x64, dtype):
    """x64 as `dtype`; the restatement of a pure copy must survive that unchanged"""
    y = x64.to(dtype)
    assert torch.equal(y.double(), x64), "the expected values are not representable in %s" % dtype
    return y


def assert_same_bits(got, expected, what):
    """EVERY element of the buffer, owned or not: the same bit pattern.  `expected` is a whole buffer: the restatement where the kernel
    owns, zero bits in the tails it must clear, the sentinel everywhere else."""
    assert got.dtype == expected.dtype and got.shape == expected.shape, (what, got.dtype, got.shape, expected.dtype, expected.shape)
    bad = bits(got) != bits(expected)
    n = int(bad.sum())
    assert n == 0, "%s: %d of %d elements differ, first at %s" % (what, n, bad.numel(), tuple(bad.nonzero()[0].tolist()))


# ---- the exact-arithmetic family of the GEMM ---------------------------------------------------------------------------------------
# (M, N, K, batch): tile 256 x 128, wave tile 128 x 64, K stage 32
GEMM_SHAPES = ((1, 1, 32, 1), (129, 65, 64, 1), (256, 128, 96, 1), (257, 129, 64, 3), (513, 127, 2048, 1), (64, 300, 32, 2))
GEMM_ALPHAS = (1.0, 0.5, -0.125)
SPLITK_CASE = (24, 40, 4, 64)          # (M, N, S, ks): S slices of ks adjacent columns of [M | N, S ks] operands
PRODUCTS = sorted({a * b for a in range(1, 5) for b in range(1, 5)})          # |a b| of two non-zero integers in [-4, 4]
PRODUCTS_SMALL = (1, 2, 4)                                                     # operands in {+-1, +-2}


def nonzero_ints(gen, shape, top):
    """integers in [-top, top] without 0"""
    mag = torch.randint(1, top + 1, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (mag * sign).double()


def gemm_exact_operands(M, N, K, batch, top=4):
    """a [batch, M, K], b [batch, N, K] fp64: non-zero integers in [-top, top].  |C| <= 16 K < 2^24 for every K here, so every partial sum
    of every accumulation order is an integer fp32 holds exactly."""
    assert top * top * K < 2 ** 24
    gen = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K + batch + top)
    return nonzero_ints(gen, (batch, M, K), top), nonzero_ints(gen, (batch, N, K), top)


def dropped_product_is_visible(exact64, alpha, dtype, products):
    """Every operand is a non-zero integer, so leaving out ANY one (m, n, k) product moves the fp64 sum of its element by one of
    +-`products`.  -> the boolean tensor [len(products) * 2, ...]: the expected output of the element without that product has other bits
    in `dtype` than the expected output."""
    want = bits((alpha * exact64).to(dtype))
    rows = []
    for v in products:
        for sgn in (1.0, -1.0):
            rows.append(bits((alpha * (exact64 - sgn * v)).to(dtype)) != want)
    return torch.stack(rows)
