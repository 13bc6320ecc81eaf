"""CPU: the restatements of tests/helpers_fp64.py against F.unfold and fp64 AUTOGRAD of the forward operation (exact, or 1e-12
relative where autograd sums in another order), and the SENSITIVITY of what test_gpu_helper_kernels.py compares with: the
exact-arithmetic GEMM operands make every single (m, n, k) product visible in the expected output, and the bit-for-bit comparison of
the data movers fails on a swapped pair of rows, on one tail column holding one 16-bit ulp and on one element moved by one 16-bit ulp."""
import pytest
import torch
import torch.nn.functional as F

import helpers_fp64 as H

REL = 1e-12
FORMATS = (torch.bfloat16, torch.float16)


def _close(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(want.abs().max())
    assert scale > 0, what
    err = float((got - want).abs().max()) / scale
    assert err < REL, "%s: %g" % (what, err)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _conv_input(x_nchw, stride, upsample):
    """what the conv sees: the nearest x2 upsample in front, the (0,1,0,1) padding of a stride-2 conv"""
    if upsample:
        x_nchw = F.interpolate(x_nchw, scale_factor=2, mode="nearest")
    return F.pad(x_nchw, (0, 1, 0, 1)) if stride == 2 else x_nchw


# ---- im2col_t ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upsample", (False, True))
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("ksize", (1, 3))
@pytest.mark.parametrize("B,Hh,W", ((1, 1, 1), (2, 5, 7), (1, 9, 12), (3, 4, 6), (1, 6, 5)))          # even and odd H and W
def test_im2col_t_equals_unfold(B, Hh, W, ksize, stride, upsample):
    g = torch.Generator().manual_seed(B * 100 + Hh * 10 + W)
    x = _rand(g, B, 5, Hh, W)
    pad = ksize // 2 if stride == 1 else 0
    if stride == 2 and ksize == 3 and not upsample and min(Hh, W) == 1:          # the padded 2-pixel side is narrower than the filter
        assert H.im2col_t(x.permute(0, 2, 3, 1).contiguous(), ksize, stride, pad, upsample).shape == (45, 0)
        return
    for pad in sorted({pad, 1} if stride == 1 else {pad}):          # stride 1: the conv's own pad k // 2, and pad 1 under either k
        want = F.unfold(_conv_input(x, stride, upsample), ksize, padding=pad, stride=stride)          # [B, C k k, L]
        want = want.permute(1, 0, 2).reshape(5 * ksize * ksize, -1)
        got = H.im2col_t(x.permute(0, 2, 3, 1).contiguous(), ksize, stride, pad, upsample)
        assert got.shape == want.shape and torch.equal(got, want)          # a pure gather: exact


# ---- the GEMM-form weight gradient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,upsample", ((1, False), (2, False), (1, True), (2, True)))
@pytest.mark.parametrize("ksize", (1, 3))
def test_gemm_of_im2col_is_the_weight_gradient(ksize, stride, upsample):
    g = torch.Generator().manual_seed(ksize * 10 + stride + 2 * upsample)
    B, Ci, Co, Hh, W = 2, 3, 4, 6, 7
    x = _rand(g, B, Ci, Hh, W)
    w, b = _rand(g, Co, Ci, ksize, ksize).requires_grad_(True), _rand(g, Co).requires_grad_(True)
    pad = ksize // 2 if stride == 1 else 0
    y = F.conv2d(_conv_input(x, stride, upsample), w, b, stride=stride, padding=pad)
    gy = _rand(g, *y.shape)
    dW, db = torch.autograd.grad((y * gy).sum(), (w, b))
    col = H.im2col_t(x.permute(0, 2, 3, 1).contiguous(), ksize, stride, pad, upsample)
    col1 = torch.cat([col, torch.ones(1, col.shape[1], dtype=torch.float64)], 0)
    gT = gy.permute(1, 0, 2, 3).reshape(Co, -1)                                                   # [Co, P], p = (b, oy, ox)
    got = H.gemm_nt(gT, col1)
    _close(got[:, :-1].reshape(Co, Ci, ksize, ksize), dW, "dW")
    _close(got[:, -1], db, "db")


# ---- dilate2 / pool2_sum -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hh,W", ((4, 6), (2, 2), (8, 10)))
def test_dilated_conv_is_the_stride2_data_gradient_for_even_sizes(Hh, W):
    """dx of the (0,1,0,1)-padded stride-2 3x3 conv = the pad-1 3x3 conv of dilate2(g) with the flipped, transposed filter.  EVEN H and W
    only: for an odd H the gradient has OH = (H - 2) // 2 + 1 rows and its dilated form 2 OH = H - 1, one short of dx."""
    g = torch.Generator().manual_seed(Hh)
    B, Ci, Co = 2, 3, 4
    x, w = _rand(g, B, Ci, Hh, W).requires_grad_(True), _rand(g, Co, Ci, 3, 3)
    y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    gy = _rand(g, *y.shape)
    dx, = torch.autograd.grad((y * gy).sum(), (x,))
    d = H.dilate2(gy.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
    assert d.shape[2:] == (Hh, W)
    _close(F.conv2d(d, w.flip(2, 3).transpose(0, 1), padding=1), dx, "dx")


def test_dilate2_zero_positions():
    g = torch.Generator().manual_seed(3)
    x = _rand(g, 2, 3, 5, 4)
    d = H.dilate2(-x.abs())                                    # all negative: a product with 0 would leave -0
    assert torch.equal(d[:, 1::2, 1::2], -x.abs())
    d[:, 1::2, 1::2] = 0
    assert int(d.view(torch.int64).abs().max()) == 0          # zero BITS


def test_pool2_sum_is_the_upsample_gradient():
    g = torch.Generator().manual_seed(4)
    x = _rand(g, 2, 3, 5, 7).requires_grad_(True)
    y = F.interpolate(x, scale_factor=2, mode="nearest")
    gy = _rand(g, *y.shape)
    dx, = torch.autograd.grad((y * gy).sum(), (x,))
    _close(H.pool2_sum(gy.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2), dx, "pool2_sum")


def test_transpose_colsum_and_the_block_split():
    g = torch.Generator().manual_seed(5)
    x = _rand(g, 2, 5, 3)
    t = H.transpose_padded(x, 64)
    assert t.shape == (2, 3, 64) and torch.equal(t[..., :5], x.transpose(1, 2))
    assert int(H.transpose_padded(-x.abs(), 64)[..., 5:].contiguous().view(torch.int64).abs().max()) == 0          # zero BITS
    _close(H.colsum(x[0]), x[0].sum(0), "colsum")
    assert [H.colsum_blocks(P) for P in (1, 511, 512, 513, 1025, 256 * 512 + 1)] == [(1, 1), (1, 511), (1, 512), (2, 257), (3, 342), (256, 513)]


@pytest.mark.parametrize("S,n", ((1, 3), (9, 5), (32, 17), (33, 4), (32, 65537)))
def test_reduce_parts_f32_order(S, n):
    """the fp32 replay against the fp64 sum (within S roundings), and the many-parts order told apart from the plain chain"""
    g = torch.Generator().manual_seed(S)
    parts = torch.randn(S, n, generator=g) * torch.exp2(torch.randint(-10, 11, (S, n), generator=g).float())
    old = torch.randn(n, generator=g)
    got = H.reduce_parts_f32(parts, 0.25, n, old)
    want = 0.25 * parts.double().sum(0) + old.double()
    tol = (S + 2) * 2.0 ** -24 * (0.25 * parts.double().abs().sum(0) + old.double().abs())
    assert got.dtype == torch.float32 and bool(((got.double() - want).abs() <= tol).all())
    assert H.many_parts(S, n) == (S >= 32 and n <= 65536)
    if S == 33:          # 33 parts: chain 0 = p0 + p16 + p32, which the plain chain adds in another order
        plain = torch.zeros(n)
        for k in range(S):
            plain = plain + parts[k]
        assert not torch.equal(H.bits(H.reduce_parts_f32(parts, 1.0, n)), H.bits(plain))


# ---- sensitivity: the exact operands of the GEMM -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", H.GEMM_SHAPES)
def test_exact_gemm_operands_show_every_single_product(shape):
    """fp32 output, every alpha: the expected value and the value without any one product are both exact in fp32 and differ.  16-bit
    output at K = 32 with operands in {+-1, +-2}: the same in both 16-bit formats.  16-bit output at a larger K (the GPU test asserts
    == the one rounding of the exact value): a dropped product is visible wherever it exceeds one 16-bit ulp of the result, which is
    all this form can promise and is asserted as such."""
    M, N, K, batch = shape
    a, b = H.gemm_exact_operands(M, N, K, batch)
    exact = H.gemm_nt(a, b)
    assert float(a.abs().min()) >= 1 and float(b.abs().min()) >= 1 and float((a.abs() @ b.abs().transpose(1, 2)).max()) < 2 ** 24
    for alpha in H.GEMM_ALPHAS:
        assert torch.equal((alpha * exact).float().double(), alpha * exact)
        assert bool(H.dropped_product_is_visible(exact, alpha, torch.float32, H.PRODUCTS).all())
    for dtype in FORMATS:
        if K == 32:
            a2, b2 = H.gemm_exact_operands(M, N, K, batch, top=2)
            e2 = H.gemm_nt(a2, b2)
            for alpha in H.GEMM_ALPHAS:
                assert torch.equal((alpha * e2).to(dtype).double(), alpha * e2)          # |C| <= 128: representable
                assert bool(H.dropped_product_is_visible(e2, alpha, dtype, H.PRODUCTS_SMALL).all())
        else:
            m = 7 if dtype == torch.bfloat16 else 10
            for v in H.PRODUCTS:          # a drop of more than one ulp16 of either value cannot round to the same bits
                for sgn in (1.0, -1.0):
                    other = exact - sgn * v
                    ulp = torch.exp2(torch.floor(torch.log2(torch.maximum(exact.abs(), other.abs()).clamp_min(1.0))) - m)
                    seen = H.bits(other.to(dtype)) != H.bits(exact.to(dtype))
                    assert bool(seen[v > ulp].all())


def test_exact_splitk_operands_show_every_single_product():
    M, N, S, ks = H.SPLITK_CASE
    a, b = H.gemm_exact_operands(M, N, S * ks, 1)
    exact = H.gemm_nt(a, b)
    assert bool(H.dropped_product_is_visible(exact, 1.0, torch.float32, H.PRODUCTS).all())
    # a slice that read one column of its neighbour adds a non-zero product: the same condition, with the other sign
    parts = H.gemm_nt(a[0].view(M, S, ks).transpose(0, 1), b[0].view(N, S, ks).transpose(0, 1))
    assert torch.equal(parts.sum(0), exact[0])


# ---- sensitivity: the comparison of the data movers --------------------------------------------------------------------------------
def _expected_buffer(dtype, rows=6, cols=40, ld=64, guard=2):
    """a transposed-operand buffer as the GPU test builds it: `guard` sentinel rows above and below, owned rows with distinct
    values in [0, cols) and zero bits in [cols, ld)"""
    g = torch.Generator().manual_seed(9)
    buf = H.sentinel16((rows + 2 * guard, ld), dtype)
    body = H.rounded_exactly(torch.randn(rows, cols, generator=g).to(dtype).double(), dtype)
    buf[guard:guard + rows, :cols] = body
    buf[guard:guard + rows, cols:] = 0
    return buf, guard, rows, cols


@pytest.mark.parametrize("dtype", FORMATS)
def test_mover_comparison_fails_on_each_corruption(dtype):
    want, guard, rows, cols = _expected_buffer(dtype)
    H.assert_same_bits(want.clone(), want, "clean")
    swapped = want.clone()
    swapped[[guard, guard + 1]] = swapped[[guard + 1, guard]]
    tail = want.clone()
    tail.view(torch.int16)[guard + 2, cols + 3] = 1                                  # one 16-bit ulp: the smallest subnormal
    moved = want.clone()
    moved.view(torch.int16)[guard + 3, 5] += 1                                       # the next value of the format
    sentinel = want.clone()
    sentinel.view(torch.int16)[0, 0] = 0                                             # a write outside what the kernel owns
    for name, bad in (("rows swapped", swapped), ("tail column", tail), ("one ulp", moved), ("sentinel", sentinel)):
        assert int((H.bits(bad) != H.bits(want)).sum()) >= 1, name
        with pytest.raises(AssertionError):
            H.assert_same_bits(bad, want, name)
    with pytest.raises(AssertionError):                                              # -0 in a tail is not zero bits
        neg = want.clone()
        neg.view(torch.int16)[guard, cols] = -0x8000
        H.assert_same_bits(neg, want, "minus zero")
