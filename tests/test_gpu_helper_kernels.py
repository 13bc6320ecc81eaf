"""GPU: the NT GEMM of csrc/gemm.hip with its two reduction kernels, and the data movers of csrc/train_ops.hip that feed it and the
data gradients (transpose, im2col_t, im2col_t_f32, dilate2, pool2_sum, add, the two casts, colsum), PER ELEMENT against the fp64
restatements of tests/helpers_fp64.py (checked on the CPU against F.unfold and fp64 autograd: test_helpers_fp64_host.py), in both
16-bit formats.  No element is left out of any comparison: every output lives in a buffer larger than what the kernel owns, filled
with a sentinel first (int16 0x7B7B; NaN for fp32), and everything outside the owned region must still hold it.  Every launch runs
twice and the two buffers must be bit-identical.

The rule is the one of fp64_bounds.py (U = 2^-24, one fp32 rounding):
    16-bit outputs   |got - exact| <= 0.5 ulp16(exact) + slack
    fp32 outputs     |got - exact| <= slack
`slack` is counted from the kernel's own expression and stated next to each call.  A pure copy must EQUAL the restatement bit for bit,
with ZERO BITS in the tail columns the contracts of include/glare_hip.h promise ("columns [P, ldp) are zero-filled", "columns
[rows, ld_out) zero-filled", "0 elsewhere").  The GEMM and the sums have two operand families, as wgrad.hip has: non-zero integers,
where every partial sum of every order is exact in fp32 and the result must EQUAL the fp64 sum (one missing or one extra product
changes it: test_helpers_fp64_host.py), and normal operands within the counted bound."""
import pytest
import torch

import helpers_fp64 as H
from fp64_bounds import U, _f32, _r16, assert_rounded
from glare_amd import _lib, ops, train_ops
from glare_amd._lib import check, ptr, stream_handle
from test_gpu_backward_edges import _reduce_depth, check_f32

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 2          # sentinel rows above and below every 2-D output


@pytest.fixture(params=("bf16", "fp16"))
def prec(request):
    with ops.use_precision(request.param):
        yield request.param


def _rup(a, b):
    return -(-a // b) * b


def _sent16(*shape):
    return H.sentinel16(shape, ops.act_dtype(), "cuda")


def _nan32(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def _sentinel_like(t):
    return _nan32(*t.shape) if t.dtype == torch.float32 else _sent16(*t.shape)


def _twice(launch):
    """launch() -> a tensor or a tuple of tensors, each a WHOLE buffer (sentinel margins included).  Runs it twice on fresh buffers and
    asserts the same bits (fixed order, no atomics) -> the first result."""
    first, second = launch(), launch()
    for a, b in zip(*((r if isinstance(r, tuple) else (r,)) for r in (first, second))):
        assert torch.equal(H.bits(a), H.bits(b)), "two runs of one launch differ"
    return first


def _refused(call, *untouched):
    """the entry point returns an error before any launch: GlareError, and the output buffers keep their sentinel"""
    with pytest.raises(_lib.GlareError):
        call()
    torch.cuda.synchronize()
    for t in untouched:
        H.assert_same_bits(t, _sentinel_like(t), "a refused call wrote to its output")


def _normal(gen, *shape):
    """N(0, 1) with |x| >= 2^-6: normal-range in both 16-bit formats, before and after rounding"""
    x = torch.randn(*shape, generator=gen)
    return _r16(torch.where(x < 0, -1.0, 1.0) * x.abs().clamp_min(2.0 ** -6))


# ---- (a) gemm_nt -------------------------------------------------------------------------------------------------------------------
def _operand(vals16, ld):
    """[batch, rows, K] 16-bit -> the same values as a row-strided view (row stride ld > K, start 32 elements into the buffer); every
    other element of the buffer is NaN, so that a read beyond K, beyond a row or beyond a batch poisons the result"""
    batch, rows, K = vals16.shape
    buf = torch.full((32 + batch * rows * ld,), NAN, dtype=ops.act_dtype(), device="cuda")
    view = buf[32:].view(batch, rows, ld)[:, :, :K]
    view.copy_(vals16)
    return view


class _C:
    """the output of one GEMM: [batch, M, N] with ldc = N + 8 and a batch stride of M ldc + 24 inside a sentinel-filled buffer"""

    def __init__(self, batch, M, N, f32, old=None):
        self.dims, self.strides = (batch, M, N), (M * (N + 8) + 24, N + 8, 1)
        n = batch * self.strides[0] + 16
        self.buf = _nan32(n) if f32 else _sent16(n)
        self.view = self.buf.as_strided(self.dims, self.strides)
        if old is not None:
            self.view.copy_(old)

    def expected(self, owned):
        """the whole buffer a correct kernel leaves: `owned` in [M] x [N] of every batch, the sentinel everywhere else"""
        e = _sentinel_like(self.buf)
        e.as_strided(self.dims, self.strides).copy_(owned)
        return e

    def outside_untouched(self, what):
        e = self.buf.clone()
        s = _sentinel_like(self.buf)
        e.as_strided(self.dims, self.strides).copy_(s.as_strided(self.dims, self.strides))
        H.assert_same_bits(e, s, what + ": written outside [M] x [N]")


def _gemm(a, b, alpha, f32, accumulate=False, old=None):
    batch, M, _ = a.shape
    N = b.shape[1]

    def launch():
        c = _C(batch, M, N, f32, old)
        r = train_ops.gemm_nt(a, b, out=c.view, alpha=alpha, out_dtype=torch.float32 if f32 else ops.act_dtype(), accumulate=accumulate)
        assert r is c.view
        launch.c = c
        return c.buf

    _twice(launch)
    return launch.c


@pytest.mark.parametrize("shape", H.GEMM_SHAPES)
def test_gemm_nt_exact_operands(prec, shape):
    """Non-zero integers in [-4, 4], alpha a power of two: every product and every partial sum is an integer below 2^24, so no
    accumulation order rounds and the fp32 output must EQUAL alpha times the fp64 sum.  A 16-bit output at K = 32 with operands in
    {+-1, +-2} (|C| <= 128: representable) must EQUAL it as well; at a larger K the fp32 value is exact and ONE rounding to nearest even
    remains: == _r16(exact)."""
    M, N, K, batch = shape
    a64, b64 = (t.cuda() for t in H.gemm_exact_operands(M, N, K, batch))
    exact = H.gemm_nt(a64, b64)
    a, b = _operand(_r16(a64), K + 64), _operand(_r16(b64), K + 32)
    assert a.stride(1) == K + 64 and b.stride(1) == K + 32 and a.data_ptr() % 64 == 0
    for alpha in H.GEMM_ALPHAS:
        c = _gemm(a, b, alpha, f32=True)
        H.assert_same_bits(c.buf, c.expected((alpha * exact).float()), "gemm_nt fp32 %s alpha %g" % (shape, alpha))
    if K == 32:
        a64, b64 = (t.cuda() for t in H.gemm_exact_operands(M, N, K, batch, top=2))
        exact = H.gemm_nt(a64, b64)
        a, b = _operand(_r16(a64), K + 64), _operand(_r16(b64), K + 32)
    for alpha in H.GEMM_ALPHAS:
        want = H.rounded_exactly(alpha * exact, ops.act_dtype()) if K == 32 else _r16(alpha * exact)
        c = _gemm(a, b, alpha, f32=False)
        H.assert_same_bits(c.buf, c.expected(want), "gemm_nt 16-bit %s alpha %g" % (shape, alpha))


@pytest.mark.parametrize("shape", H.GEMM_SHAPES)
def test_gemm_nt_random_operands(prec, shape):
    """Normal operands (normal-range in the 16-bit format: what the MFMA does with 16-bit subnormals is not asserted), alpha = ln 2 as
    the C float.  v = alpha * acc: one rounding per accumulated product, as the project counts MFMA chains (K), and the alpha product
    (1): slack_v = (K + 1) U |alpha| sum_k |a| |b|.  accumulate: fp32 `v + old` rounds once on |old| + |v| (v within slack_v of its
    exact value); the 16-bit form reads the old value exactly, adds in fp32 (the same one U) and then rounds to 16 bits."""
    M, N, K, batch = shape
    gen = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    a16, b16 = _normal(gen, batch, M, K).cuda(), _normal(gen, batch, N, K).cuda()
    alpha = _f32(0.6931471805599453)
    a, b = _operand(a16, K + 64), _operand(b16, K + 32)
    v = H.gemm_nt(a16.double(), b16.double(), alpha)
    slack_v = (K + 1) * U * abs(alpha) * H.gemm_nt(a16.double().abs(), b16.double().abs())
    tag = "gemm_nt:%s" % "x".join(str(s) for s in shape)
    old32 = torch.randn(batch, M, N, generator=gen).cuda()
    for f32 in (True, False):
        for accumulate in (False, True):
            old = None if not accumulate else (old32 if f32 else _r16(old32))
            c = _gemm(a, b, alpha, f32, accumulate, old)
            exact = v if old is None else v + old.double()
            slack = slack_v if old is None else slack_v + U * (old.double().abs() + v.abs() + slack_v)
            t = "%s:%s%s" % (tag, "f32" if f32 else "16", ":acc" if accumulate else "")
            (check_f32 if f32 else assert_rounded)(c.view.contiguous(), exact, slack, t)
            c.outside_untouched(t)


def test_gemm_nt_split_k_slices(prec):
    """The form conv_weight_grad builds: S slices of ks ADJACENT columns of dense [rows, S ks] operands as the batch axis
    (as_strided), a partial C per slice, then reduce_parts.  Integer operands: every partial and their sum must EQUAL the fp64 sums -- a
    slice that read one column of its neighbour would add a non-zero integer."""
    M, N, S, ks = H.SPLITK_CASE
    a64, b64 = (t[0].cuda() for t in H.gemm_exact_operands(M, N, S * ks, 1))
    a16, b16 = _r16(a64), _r16(b64)
    a3 = a16.as_strided((S, M, ks), (ks, S * ks, 1))
    b3 = b16.as_strided((S, N, ks), (ks, S * ks, 1))
    c = _gemm(a3, b3, 1.0, f32=True)
    parts64 = H.gemm_nt(a64.view(M, S, ks).transpose(0, 1), b64.view(N, S, ks).transpose(0, 1))
    H.assert_same_bits(c.buf, c.expected(parts64.float()), "split-K partials")
    total = _twice(lambda: train_ops.reduce_parts(c.view.contiguous(), out=_nan32(M, N)))
    assert torch.equal(total.double(), H.gemm_nt(a64, b64))


def _gemm_raw(A, B, C, M, N, K, lda, ldb, ldc, batch=1):
    check(_lib.lib().glare_gemm_nt_bf16(A, B, C, M, N, K, lda, ldb, ldc, batch, 0, 0, 0, 1.0, 0, 0, stream_handle()), "glare_gemm_nt_bf16")


def test_gemm_nt_refusals(prec):
    """Every argument the entry point checks itself, refused BEFORE a launch (nothing else is passed in: an unchecked argument would
    be a wild launch, not a refusal).  M = 0 is no error: it returns without touching C."""
    a = torch.ones(8, 128, dtype=ops.act_dtype(), device="cuda")
    b = torch.ones(8, 128, dtype=ops.act_dtype(), device="cuda")
    c = _nan32(8, 16)
    A, B, C = ptr(a), ptr(b), ptr(c)
    _refused(lambda: _gemm_raw(A, B, C, 8, 8, 48, 128, 128, 16), c)                      # K % 32 != 0
    _refused(lambda: _gemm_raw(A, B, C, 8, 8, 0, 128, 128, 16), c)                       # K == 0
    _refused(lambda: _gemm_raw(A, B, C, 8, 8, 32, 36, 128, 16), c)                       # lda % 8 != 0
    _refused(lambda: _gemm_raw(A, B, C, 8, 8, 64, 32, 128, 16), c)                       # lda < K
    _refused(lambda: _gemm_raw(A, B, C, 8, 8, 32, 128, 128, 4), c)                       # ldc < N
    assert (A + 8) % 8 == 0 and (A + 8) % 16 != 0
    _refused(lambda: _gemm_raw(A + 8, B, C, 8, 8, 32, 64, 128, 16), c)                   # A 8-byte but not 16-byte aligned
    _refused(lambda: _gemm_raw(A, B, C, 1, 1, 32, 128, 128, 16, batch=65536), c)         # the grid's y limit
    _gemm_raw(A, B, C, 0, 8, 32, 128, 128, 16)                                           # M == 0: nothing to do
    torch.cuda.synchronize()
    H.assert_same_bits(c, _sentinel_like(c), "M == 0 wrote to C")
    _gemm_raw(A, B, C, 8, 8, 32, 128, 128, 16)                                           # and the same arguments, valid: 32 ones each
    assert torch.equal(c[:, :8], torch.full((8, 8), 32.0, device="cuda")) and bool(torch.isnan(c[:, 8:]).all())


# ---- (b) reduce_parts --------------------------------------------------------------------------------------------------------------
REDUCE_CASES = ([(s, n) for s in (1, 7, 8, 9, 17) for n in (1, 255, 257)]             # the plain chain: the 8-wide unrolled loop and its tail
                + [(s, n) for s in (32, 33, 256) for n in (1, 15, 16, 17, 576)]       # many parts of few elements: 16 elements per block
                + [(32, 65536), (32, 65537)])                                          # the boundary of the selection
GROUPS = 3


@pytest.mark.parametrize("S,n", REDUCE_CASES)
def test_reduce_parts_grouped_bits_and_bound(S, n):
    """glare_reduce_parts_grouped_f32, three groups, scale in {1, 0.25}, accumulating or not.  Random fp32 parts spanning 2^-10..2^10
    must be BIT-EQUAL to the fp32 replay of the documented order (helpers_fp64.reduce_parts_f32), and within (_reduce_depth + 2) U of the
    fp64 sum on the magnitudes of the terms: the additions behind an element, the scale product and the accumulating addition."""
    gen = torch.Generator().manual_seed(S * 100003 + n)
    parts = (torch.randn(GROUPS, S, n, generator=gen) * torch.exp2(torch.randint(-10, 11, (GROUPS, S, n), generator=gen).float()))
    old = torch.randn(GROUPS, n, generator=gen)
    parts_d = parts.cuda()
    assert _reduce_depth(S, n) == (-(-S // 16) + 15 if H.many_parts(S, n) else S)          # the count agrees with the kernel chosen
    for scale in (1.0, 0.25):
        for accumulate in (0, 1):
            def launch():
                out = _nan32(GROUPS * n + 32)
                if accumulate:
                    out[:GROUPS * n] = old.reshape(-1).cuda()
                check(_lib.lib().glare_reduce_parts_grouped_f32(ptr(parts_d), GROUPS, S, n, scale, ptr(out), accumulate, stream_handle()),
                      "glare_reduce_parts_grouped_f32")
                return out
            out = _twice(launch).cpu()
            replay = torch.stack([H.reduce_parts_f32(parts[g], scale, n, old[g] if accumulate else None) for g in range(GROUPS)])
            want = torch.cat([replay.reshape(-1), torch.full((32,), NAN)])
            H.assert_same_bits(out, want, "reduce_parts %dx%d scale %g acc %d" % (S, n, scale, accumulate))
            exact = scale * parts.double().sum(1) + (old.double() if accumulate else 0.0)
            mags = scale * parts.double().abs().sum(1) + (old.double().abs() if accumulate else 0.0)
            check_f32(out[:GROUPS * n].view(GROUPS, n), exact, (_reduce_depth(S, n) + 2) * U * mags, "reduce_parts:%dx%d" % (S, n))


# ---- (c) transpose -----------------------------------------------------------------------------------------------------------------
TRANSPOSE_SHAPES = ((1, 1, 1), (1, 63, 8), (2, 65, 72), (1, 130, 20))          # (batch, R, C)


def _transpose_input(vals16, form):
    """[batch, R, C] -> a view of a NaN-filled buffer: "vec" (ld_in % 8 == 0, 16-byte aligned: the vector path, with a scalar last
    chunk when C % 8 != 0), "off1" (the view starts one element into its buffer) and "ld20" (ld_in = 20): vec_ok == 0"""
    batch, R, C = vals16.shape
    ld, off = {"vec": (_rup(C, 8) + 8, 0), "off1": (_rup(C, 8) + 8, 1), "ld20": (20, 0)}[form]
    buf = torch.full((off + batch * R * ld,), NAN, dtype=ops.act_dtype(), device="cuda")
    view = buf[off:].view(batch, R, ld)[:, :, :C]
    view.copy_(vals16)
    return view


@pytest.mark.parametrize("shape,form", [(s, f) for s in TRANSPOSE_SHAPES for f in ("vec", "off1", "ld20") if f != "ld20" or s[2] <= 20])
def test_transpose_equals_and_zero_fills(prec, shape, form):
    batch, R, C = shape
    gen = torch.Generator().manual_seed(R * 100 + C)
    vals = _r16(torch.randn(batch, R, C, generator=gen)).cuda()
    x = _transpose_input(vals, form)
    assert (x.data_ptr() % 16 == 0 and x.stride(1) % 8 == 0) == (form == "vec")
    for ld_out in (_rup(R, 64), _rup(R, 64) + 128):
        want = _sent16(batch, C + 2 * GUARD, ld_out)
        want[:, GUARD:GUARD + C] = H.rounded_exactly(H.transpose_padded(vals.double(), ld_out), ops.act_dtype())
        assert ld_out > R and int(H.bits(want[:, GUARD:GUARD + C, R:]).abs().max()) == 0          # +0: zero bits

        def launch():
            buf = _sent16(batch, C + 2 * GUARD, ld_out)
            train_ops.transpose(x, out=buf[:, GUARD:GUARD + C])
            return buf
        H.assert_same_bits(_twice(launch), want, "transpose %s %s ld_out %d" % (shape, form, ld_out))


def test_transpose_refusals(prec):
    x = torch.ones(65, 8, dtype=ops.act_dtype(), device="cuda")
    out = _sent16(8, 128)
    lib = _lib.lib()
    for ld_in, ld_out in ((8, 96), (8, 64), (4, 128)):          # ld_out % 64 != 0; ld_out < R; ld_in < C
        _refused(lambda: check(lib.glare_transpose_bf16(ptr(x), ld_in, 0, ptr(out), ld_out, 0, 65, 8, 1, stream_handle()), "glare_transpose_bf16"), out)


# ---- (d) im2col_t ------------------------------------------------------------------------------------------------------------------
IM2COL_INPUTS = ((1, 1, 1), (2, 5, 7), (1, 9, 12), (3, 4, 6))                                        # (B, H, W): odd and even sides
IM2COL_CHANNELS = {"vec": (8, 8, 0), "vec+tail": (20, 32, 8), "pitch12": (12, 12, 0), "off4": (8, 16, 4), "two tiles": (72, 72, 0)}


def _nhwc_window(gen, B, Hh, W, Ci, pitch, off):
    """x [B, H, W, pitch] 16-bit on the device with Ci random channels at `off` and NaN in every other channel -> (x, the window as fp64)"""
    vals = _r16(torch.randn(B, Hh, W, Ci, generator=gen))
    x = torch.full((B, Hh, W, pitch), NAN, dtype=ops.act_dtype())
    x[..., off:off + Ci] = vals
    return x.cuda(), vals.double()


def _col_expected(blocks, ldp, ones_row_P=None):
    """the whole col buffer: GUARD sentinel rows, then each [rows, P] block with zero bits in [P, ldp), then (ones_row_P = P) the row that
    is 1 for p < P and 0 beyond, then GUARD sentinel rows"""
    rows = sum(b.shape[0] for b in blocks) + (ones_row_P is not None)
    want = H.sentinel16((rows + 2 * GUARD, ldp), ops.act_dtype())
    r = GUARD
    for b in blocks:
        want[r:r + b.shape[0]] = 0
        want[r:r + b.shape[0], :b.shape[1]] = H.rounded_exactly(b, ops.act_dtype())
        r += b.shape[0]
    if ones_row_P is not None:
        want[r] = 0
        want[r, :ones_row_P] = 1
    return want


@pytest.mark.parametrize("channels", sorted(IM2COL_CHANNELS))
@pytest.mark.parametrize("bhw", IM2COL_INPUTS)
def test_im2col_t_equals_and_zero_fills(prec, bhw, channels):
    """k in {1, 3} x stride 1 (pad k // 2) and stride 2 (the (0,1,0,1) padding) x the nearest x2 upsample on / off x two ldp, with the
    ones row: a pure copy, so the whole buffer must EQUAL the restatement, the tail columns [P, ldp) and the ones row beyond P zero bits."""
    B, Hh, W = bhw
    Ci, pitch, off = IM2COL_CHANNELS[channels]
    gen = torch.Generator().manual_seed(B * 1000 + Hh * 10 + W + Ci)
    x, win = _nhwc_window(gen, B, Hh, W, Ci, pitch, off)
    assert (pitch % 8 == 0 and off % 8 == 0) == (channels in ("vec", "vec+tail", "two tiles"))          # vec_ok
    ran = 0
    for ksize in (1, 3):
        for stride in (1, 2):
            for ups in (False, True):
                pad = ksize // 2 if stride == 1 else 0
                ref = H.im2col_t(win, ksize, stride, pad, ups)
                rows, P = ref.shape
                if P == 0:          # the padded side is narrower than the filter: no output pixel, refused
                    buf = _sent16(rows + 1 + 2 * GUARD, 64)
                    _refused(lambda: train_ops.im2col_t(x, ksize, stride, pad, ups, cin=Ci, in_off=off, ldp=64, col=buf, row_base=GUARD,
                                                        ones_row=GUARD + rows), buf)
                    continue
                for ldp in (_rup(P, 64), _rup(P, 128) + 64):
                    def launch():
                        buf = _sent16(rows + 1 + 2 * GUARD, ldp)
                        train_ops.im2col_t(x, ksize, stride, pad, ups, cin=Ci, in_off=off, ldp=ldp, col=buf, row_base=GUARD, ones_row=GUARD + rows)
                        return buf
                    H.assert_same_bits(_twice(launch).cpu(), _col_expected([ref], ldp, P),
                                       "im2col_t %s %s k%d s%d ups%d ldp %d" % (bhw, channels, ksize, stride, ups, ldp))
                    ran += 1
    assert ran == (14 if bhw == (1, 1, 1) else 16)          # 1 x 1 under the stride-2 3x3 without the upsample has no output


@pytest.mark.parametrize("stride,ups", ((1, False), (2, True)))
def test_im2col_t_two_sources(prec, stride, ups):
    """torch.cat((x, x2), 1) as the conv's input: the second call writes at row_base = c1 k k of the same buffer.  Both row ranges must be
    exact and the sentinel rows around them untouched."""
    B, Hh, W, k = 2, 5, 7, 3
    gen = torch.Generator().manual_seed(77 + stride)
    (c1, p1, o1), (c2, p2, o2) = IM2COL_CHANNELS["vec"], IM2COL_CHANNELS["vec+tail"]
    x1, w1 = _nhwc_window(gen, B, Hh, W, c1, p1, o1)
    x2, w2 = _nhwc_window(gen, B, Hh, W, c2, p2, o2)
    pad = 1 if stride == 1 else 0
    r1, r2 = H.im2col_t(w1, k, stride, pad, ups), H.im2col_t(w2, k, stride, pad, ups)
    P, rows = r1.shape[1], (c1 + c2) * k * k
    ldp = _rup(P, 64) + 64

    def launch():
        buf = _sent16(rows + 1 + 2 * GUARD, ldp)
        train_ops.im2col_t(x1, k, stride, pad, ups, cin=c1, in_off=o1, ldp=ldp, col=buf, row_base=GUARD, ones_row=GUARD + rows)
        train_ops.im2col_t(x2, k, stride, pad, ups, cin=c2, in_off=o2, ldp=ldp, col=buf, row_base=GUARD + c1 * k * k)
        return buf
    H.assert_same_bits(_twice(launch).cpu(), _col_expected([r1, r2], ldp, P), "im2col_t two sources")


def test_im2col_t_refusals(prec):
    x = torch.ones(1, 4, 4, 8, dtype=ops.act_dtype(), device="cuda")
    buf = _sent16(80, 128)
    lib = _lib.lib()

    def call(ksize, stride, ldp):
        return lambda: check(lib.glare_im2col_t_bf16(ptr(x), 1, 4, 4, 8, 0, 8, ksize, stride, ksize // 2, 0, ptr(buf), ldp, 0, -1, stream_handle()),
                             "glare_im2col_t_bf16")
    _refused(call(3, 1, 96), buf)          # ldp % 64 != 0
    _refused(call(3, 1, 0), buf)           # ldp < P = 16
    _refused(call(2, 1, 64), buf)          # ksize = 2
    _refused(call(3, 3, 64), buf)          # stride = 3


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("bhw", ((1, 1, 1), (2, 5, 7)))
def test_im2col_t_f32_equals_the_rounded_gather(prec, bhw, layout):
    """glare_im2col_t_f32, Ci = 3, addressed by element strides: the matrix of the 16-bit form from _r16(x), k in {1, 3} (pad k // 2), ldp
    in {P rounded to 64, 320}, with and without the ones row (an ABSOLUTE row, like the 16-bit form's)."""
    B, Hh, W = bhw
    Ci = 3
    gen = torch.Generator().manual_seed(B + Hh + W)
    x_nhwc = torch.randn(B, Hh, W, Ci, generator=gen)
    x = (x_nhwc.permute(0, 3, 1, 2).contiguous() if layout == "nchw" else x_nhwc).cuda()
    strides = (Ci * Hh * W, Hh * W, W, 1) if layout == "nchw" else (Hh * W * Ci, 1, W * Ci, Ci)          # (b, c, y, x)
    P = B * Hh * W
    for ksize in (1, 3):
        ref = H.im2col_t(_r16(x_nhwc).double(), ksize, 1, ksize // 2, False)
        rows = ref.shape[0]
        for ldp in (_rup(P, 64), 320):
            for ones in (False, True):
                def launch():
                    buf = _sent16(rows + 1 + 2 * GUARD, ldp)
                    check(_lib.lib().glare_im2col_t_f32(ptr(x), *strides, B, Hh, W, Ci, ksize, ksize // 2, ptr(buf), ldp, GUARD,
                                                        GUARD + rows if ones else -1, stream_handle()), "glare_im2col_t_f32")
                    return buf
                want = _col_expected([ref], ldp, P)
                if not ones:
                    want[GUARD + rows] = H.sentinel16((ldp,), ops.act_dtype())
                H.assert_same_bits(_twice(launch).cpu(), want, "im2col_t_f32 %s %s k%d ldp %d ones %d" % (bhw, layout, ksize, ldp, ones))


# ---- (e) dilate2, pool2_sum, add ---------------------------------------------------------------------------------------------------
SMALL_MAPS = ((1, 1, 1, 8), (2, 3, 5, 24), (1, 7, 2, 264))          # (B, OH, OW, C): one vector; three per pixel; 33 per pixel, > 1 block
TAIL = 64                                                           # sentinel elements behind every flat output


def _flat_out(n):
    return _sent16(n + TAIL)


def _flat_expected(owned16):
    return torch.cat([owned16.reshape(-1), _sent16(TAIL)])


def _ints(gen, *shape):
    return _r16(torch.randint(-4, 5, shape, generator=gen).float())


@pytest.mark.parametrize("shape", SMALL_MAPS)
def test_dilate2_equals_and_zero_fills(prec, shape):
    B, OH, OW, C = shape
    g = _r16(torch.randn(*shape, generator=torch.Generator().manual_seed(OH * OW + C))).cuda()
    want = H.rounded_exactly(H.dilate2(g.double()), ops.act_dtype())
    zero = torch.ones(2 * OH, 2 * OW, dtype=torch.bool, device="cuda")
    zero[1::2, 1::2] = False
    assert int(H.bits(want[:, zero]).abs().max()) == 0 and int(zero.sum()) == 3 * OH * OW          # "0 elsewhere": zero bits

    def launch():
        out = _flat_out(want.numel())
        check(_lib.lib().glare_dilate2_bf16(ptr(g), ptr(out), B, OH, OW, C, stream_handle()), "glare_dilate2_bf16")
        return out
    H.assert_same_bits(_twice(launch), _flat_expected(want), "dilate2 %s" % (shape,))
    H.assert_same_bits(train_ops.dilate2(g), want, "dilate2 wrapper")


@pytest.mark.parametrize("shape", SMALL_MAPS)
def test_pool2_sum_per_element(prec, shape):
    """(a0 + a1) + (a2 + a3) in fp32, rounded once to 16 bits: three additions on sum |terms|.  Integers in [-4, 4]: every sum exact, EQUAL."""
    B, Hh, W, C = shape
    gen = torch.Generator().manual_seed(Hh * W + C)

    def run(g):
        def launch():
            out = _flat_out(B * Hh * W * C)
            check(_lib.lib().glare_pool2_sum_bf16(ptr(g), ptr(out), B, Hh, W, C, stream_handle()), "glare_pool2_sum_bf16")
            return out
        out = _twice(launch)
        H.assert_same_bits(out[B * Hh * W * C:], _sent16(TAIL), "pool2_sum wrote behind its output")
        owned = out[:B * Hh * W * C].view(B, Hh, W, C)
        H.assert_same_bits(train_ops.pool2_sum(g), owned, "pool2_sum wrapper")
        return owned

    g = _ints(gen, B, 2 * Hh, 2 * W, C).cuda()
    H.assert_same_bits(run(g), H.rounded_exactly(H.pool2_sum(g.double()), ops.act_dtype()), "pool2_sum integers %s" % (shape,))
    g = _normal(gen, B, 2 * Hh, 2 * W, C).cuda()
    assert_rounded(run(g), H.pool2_sum(g.double()), 3 * U * H.pool2_sum(g.double().abs()), "pool2_sum:%s" % "x".join(str(s) for s in shape))


@pytest.mark.parametrize("three", (False, True))
@pytest.mark.parametrize("n", (8, 2040, 2056))          # one vector; 255 and 257 vectors: the last thread of a block, the second block
def test_add_per_element(prec, n, three):
    """a + b + c left to right in fp32 (c absent: + 0, exact), rounded once to 16 bits: two additions on the magnitudes."""
    gen = torch.Generator().manual_seed(n + three)

    def run(ops3):
        def launch():
            out = _flat_out(n)
            check(_lib.lib().glare_add_bf16(*(ptr(t) for t in ops3), ptr(out), n, stream_handle()), "glare_add_bf16")
            return out
        out = _twice(launch)
        H.assert_same_bits(out[n:], _sent16(TAIL), "add wrote behind its output")
        H.assert_same_bits(train_ops.add_bf16(*ops3), out[:n], "add wrapper")
        return out[:n]

    for family in (_ints, _normal):
        a, b, c = (family(gen, n).cuda() for _ in range(3))
        ops3 = (a, b, c if three else None)
        exact = a.double() + b.double() + (c.double() if three else 0.0)
        got = run(ops3)
        if family is _ints:
            H.assert_same_bits(got, H.rounded_exactly(exact, ops.act_dtype()), "add integers %d" % n)
        else:
            mags = a.double().abs() + b.double().abs() + (c.double().abs() if three else 0.0)
            assert_rounded(got, exact, 2 * U * mags, "add:%d:%d" % (n, 3 if three else 2))


def test_small_map_refusals(prec):
    lib = _lib.lib()
    g = torch.ones(1, 2, 2, 12, dtype=ops.act_dtype(), device="cuda")
    out = _sent16(4 * 4 * 12)
    _refused(lambda: check(lib.glare_dilate2_bf16(ptr(g), ptr(out), 1, 2, 2, 12, stream_handle()), "glare_dilate2_bf16"), out)       # C % 8 != 0
    _refused(lambda: check(lib.glare_pool2_sum_bf16(ptr(g), ptr(out), 1, 1, 1, 12, stream_handle()), "glare_pool2_sum_bf16"), out)   # C % 8 != 0
    _refused(lambda: check(lib.glare_add_bf16(ptr(g), ptr(g), None, ptr(out), 12, stream_handle()), "glare_add_bf16"), out)          # n % 8 != 0


def test_pool2_sum_wrapper_refuses_odd_sides(prec):
    """The kernel indexes its input as [B][2H][2W]: a floored odd side would shift every image after the first.  The wrapper says so."""
    for shape in ((2, 3, 4, 8), (2, 4, 5, 8)):
        with pytest.raises(AssertionError, match="odd side"):
            train_ops.pool2_sum(torch.ones(*shape, dtype=ops.act_dtype(), device="cuda"))


# ---- (f) the casts -----------------------------------------------------------------------------------------------------------------
def _cast_table():
    """fp32 values at the edges of the 16-bit format in use"""
    if ops.act_dtype() == torch.bfloat16:
        sub, top, edge = 2.0 ** -133, (2.0 - 2.0 ** -7) * 2.0 ** 127, (2.0 - 2.0 ** -8) * 2.0 ** 127
    else:
        sub, top, edge = 2.0 ** -24, 65504.0, 65520.0
    # sub: the smallest subnormal (half of it ties to even, 0); top: the largest finite value; edge = top + half an ulp: the tie, to inf
    assert float(torch.tensor(top, dtype=ops.act_dtype())) == top == torch.finfo(ops.act_dtype()).max
    edge, inf = torch.tensor(edge, dtype=torch.float32), torch.tensor(float("inf"))
    vals = [0.0, -0.0, sub, -sub, sub / 2, -sub / 2, 1.5 * sub, top, -top, float(torch.nextafter(edge, -inf)), float(edge),
            float(torch.nextafter(edge, inf)), -float(torch.nextafter(edge, inf)), float("inf"), -float("inf"), NAN]
    return torch.tensor(vals, dtype=torch.float32)


def _same_bits_or_nan(got, want, what):
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what + ": NaN positions"
    H.assert_same_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want), what)


@pytest.mark.parametrize("C", (1, 3, 8, 13))
@pytest.mark.parametrize("pixels", (1, 37, 300))
def test_casts_bit_for_bit(prec, pixels, C):
    """Both raw entry points with differing pitches and offsets (C channels read at offset 2 of pitch C + 4, written at offset 5 of
    pitch C + 13): fp32 -> 16 must equal x.to(dtype) on the CPU (round to nearest even, subnormals kept, the tie above the largest
    finite value to inf), 16 -> fp32 must equal .float(); NaN by isnan.  Outside the [off, off + C) window the sentinel stays."""
    dt = ops.act_dtype()
    ip, io, op_, oo = C + 4, 2, C + 13, 5
    gen = torch.Generator().manual_seed(pixels * 16 + C)
    vals = (torch.randn(pixels, C, generator=gen) * torch.exp2(torch.randint(-20, 16, (pixels, C), generator=gen).float())).reshape(-1)
    table = _cast_table()
    k = min(vals.numel(), table.numel())
    start = int(torch.randint(0, table.numel(), (1,), generator=gen))          # small cases see a rotating part of the table
    vals[:k] = table.roll(-start)[:k]
    vals = vals.view(pixels, C)
    lib = _lib.lib()
    # fp32 -> 16
    src = torch.full((pixels, ip), NAN)
    src[:, io:io + C] = vals
    src_d = src.cuda()
    want = H.sentinel16((pixels, op_), dt)
    want[:, oo:oo + C] = vals.to(dt)

    def down():
        out = _sent16(pixels, op_)
        check(lib.glare_cast_f32_bf16(ptr(src_d), ip, io, ptr(out), op_, oo, pixels, C, stream_handle()), "glare_cast_f32_bf16")
        return out
    _same_bits_or_nan(_twice(down).cpu(), want, "cast f32 -> 16 %dx%d" % (pixels, C))
    # 16 -> fp32: every 16-bit value the first cast produced (subnormals, the largest finite value, +-inf, NaN, +-0 among them)
    v16 = vals.to(dt)
    src16 = H.sentinel16((pixels, ip), dt)
    src16[:, io:io + C] = v16
    src16_d = src16.cuda()
    want32 = torch.full((pixels, op_), NAN)
    want32[:, oo:oo + C] = v16.float()

    def up():
        out = _nan32(pixels, op_)
        check(lib.glare_cast_bf16_f32(ptr(src16_d), ip, io, ptr(out), op_, oo, pixels, C, stream_handle()), "glare_cast_bf16_f32")
        return out
    got32 = _twice(up).cpu()
    inside = torch.zeros(pixels, op_, dtype=torch.bool)
    inside[:, oo:oo + C] = True
    H.assert_same_bits(got32[~inside], want32[~inside], "cast 16 -> f32 wrote outside its window")
    _same_bits_or_nan(got32[inside], want32[inside], "cast 16 -> f32 %dx%d" % (pixels, C))
    # the wrappers: extra channels of the widened 16-bit tensor are zero bits; the narrowing read drops them
    wide = train_ops.cast_to_bf16(vals.cuda(), pitch=C + 3).cpu()
    _same_bits_or_nan(wide, torch.cat([vals.to(dt), torch.zeros(pixels, 3, dtype=dt)], 1), "cast_to_bf16")
    _same_bits_or_nan(train_ops.cast_to_f32(wide.cuda(), C=C).cpu(), v16.float(), "cast_to_f32")


# ---- (g) colsum --------------------------------------------------------------------------------------------------------------------
COLSUM_P = (1, 511, 512, 513, 1025, 256 * 512 + 1)          # one block up to its 512 pixels; two; three; the 256-block cap, per = 513


def _colsum_raw(g2d, C, ws_floats=None):
    P = g2d.shape[0]
    blocks, _ = H.colsum_blocks(P)
    n = blocks * C if ws_floats is None else ws_floats
    out, ws = _nan32(C + 16), _nan32(n + 16)
    check(_lib.lib().glare_colsum_bf16(ptr(g2d), g2d.stride(0), P, C, ptr(out), ptr(ws), n * 4, stream_handle()), "glare_colsum_bf16")
    return out, ws


@pytest.mark.parametrize("C", (1, 8, 257))          # 257: two channel blocks
@pytest.mark.parametrize("P", COLSUM_P)
def test_colsum_per_element(prec, P, C):
    """A row-strided view with pitch = C + 8 (NaN in the other columns).  A block's chain over its `per` pixels, then reduce_parts over the
    blocks: (per + _reduce_depth(blocks, C)) U sum |g|.  Integers |g| <= 4: every partial below 2^24, EQUAL."""
    blocks, per = H.colsum_blocks(P)
    gen = torch.Generator(device="cuda").manual_seed(P + C)
    for family in ("integers", "normal"):
        buf = torch.full((P, C + 8), NAN, dtype=ops.act_dtype(), device="cuda")
        if family == "integers":
            buf[:, :C] = torch.randint(-4, 5, (P, C), generator=gen, device="cuda").to(ops.act_dtype())
        else:
            buf[:, :C] = torch.randn(P, C, generator=gen, device="cuda").to(ops.act_dtype())
        g = buf[:, :C]
        out, ws = _twice(lambda: _colsum_raw(g, C))
        assert bool(torch.isnan(out[C:]).all()) and bool(torch.isnan(ws[blocks * C:]).all()), "colsum wrote outside its output / workspace"
        g64 = g.double()
        if family == "integers":
            assert torch.equal(out[:C].double(), H.colsum(g64))
        else:
            check_f32(out[:C], H.colsum(g64), (per + _reduce_depth(blocks, C)) * U * H.colsum(g64.abs()), "colsum:%dx%d" % (P, C))
        assert torch.equal(H.bits(train_ops.colsum(g, C)), H.bits(out[:C]))


def test_colsum_refusals(prec):
    buf = torch.ones(1025, 16, dtype=ops.act_dtype(), device="cuda")
    out, ws = _nan32(24), _nan32(64)
    lib = _lib.lib()
    _refused(lambda: check(lib.glare_colsum_bf16(ptr(buf), 4, 1025, 8, ptr(out), ptr(ws), 256, stream_handle()), "glare_colsum_bf16"), out, ws)          # pitch < C
    blocks, _ = H.colsum_blocks(1025)
    _refused(lambda: check(lib.glare_colsum_bf16(ptr(buf), 16, 1025, 8, ptr(out), ptr(ws), (blocks * 8 - 1) * 4, stream_handle()), "glare_colsum_bf16"),
             out, ws)                                                                                                                               # one float short


# ---- (h) the composite: conv_weight_grad through the im2col form ----------------------------------------------------------------------
# (Cin, Cout, H, W) of one image under the stride-2 3x3 -> (swap, S): Cout on the GEMM's 128 side with two K slices of 2048 pixels; the
# un-swapped single GEMM
WGRAD_GEMM_CASES = {(16, 24, 128, 128): (True, 2), (8, 136, 64, 96): (False, 1)}


@pytest.mark.parametrize("case", sorted(WGRAD_GEMM_CASES))
def test_conv_weight_grad_gemm_form(prec, case, monkeypatch):
    """im2col_t (stride 2) + transpose + split-K gemm_nt + reduce_parts, wgrad.hip not involved.  Integer operands: (dW, db) must EQUAL the
    fp64 gemm_nt(g^T, [im2col_t(x); ones]).  Normal operands: the MFMA chain over the ks pixels of a slice, the chain over the S partials
    and the scale product of reduce_parts: (ks + S + 1) U sum |terms|.  The branch (swap, S) is asserted from what reached gemm_nt."""
    Ci, Co, Hh, W = case
    swap, S = WGRAD_GEMM_CASES[case]
    OH, OW = H.conv_out_size(Hh, 3, 2, 0), H.conv_out_size(W, 3, 2, 0)
    P, n_rows = OH * OW, Ci * 9
    seen = []
    real = train_ops.gemm_nt
    monkeypatch.setattr(train_ops, "gemm_nt", lambda a, b, **kw: (seen.append((tuple(a.shape), tuple(b.shape))), real(a, b, **kw))[1])
    gen = torch.Generator().manual_seed(Ci + Co)
    for family in (_ints, _normal):
        x = family(gen, 1, Hh, W, Ci).cuda()
        g = family(gen, 1, OH, OW, Co).cuda()

        def run():
            del seen[:]
            r = train_ops.conv_weight_grad(lambda ldp, ones_row: train_ops.im2col_t(x, 3, 2, ldp=ldp, ones_row=ones_row), g, Co, n_rows)
            return r
        got = run()
        ks = _rup(P, 64 * S) // S
        a_shape, b_shape = (S, Co, ks), (S, n_rows + 1, ks)
        assert seen == [(b_shape, a_shape) if swap else (a_shape, b_shape)], (seen, swap, S)
        assert got.shape == (Co, n_rows + 1) and got.is_contiguous() == (not swap)
        assert torch.equal(H.bits(run()), H.bits(got))
        col1 = torch.cat([H.im2col_t(x.double(), 3, 2, 0, False), torch.ones(1, P, dtype=torch.float64, device="cuda")], 0)
        gT = g.double().view(P, Co).t()
        exact = H.gemm_nt(gT, col1)
        if family is _ints:
            assert float(H.gemm_nt(gT.abs(), col1.abs()).max()) < 2 ** 24
            assert torch.equal(got.double(), exact)
        else:
            check_f32(got.contiguous(), exact, (ks + S + 1) * U * H.gemm_nt(gT.abs(), col1.abs()), "conv_weight_grad:%s" % "x".join(str(v) for v in case))
