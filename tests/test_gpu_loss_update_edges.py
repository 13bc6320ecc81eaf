"""GPU: the kernels that decide what a training step optimises and how the parameters then move -- csrc/loss_ops.hip (clamp, 2x2
average pool, SSIM forward / backward, 2x2 max pool forward / backward, feature MSE forward / backward), the pixel losses and the
sigmoid of csrc/train_ops.hip, Adam through its four entry points, adam_prepare, grad_nonfinite and the grad scaler's update --
PER ELEMENT against the fp64 restatements of tests/loss_fp64.py (themselves checked on the CPU: test_loss_fp64_host.py), at the
shapes where their index arithmetic changes regime: one element, a sample boundary inside a block, the second (fifth, 17th) trip
of every grid-stride loop, ragged and odd sizes, windows shrunk down to one pixel.  No element is left out of any comparison.

The bounds follow fp64_bounds.py unchanged:
    16-bit outputs   |got - exact| <= 0.5 ulp16(exact) + slack
    fp32 outputs     |got - exact| <= slack
`slack` is counted from the kernel's own expression.  For the longer expressions (SSIM, Adam) the counting is done by `V`, a value
with its running error bound: the test writes the kernel's expression once more, in the kernel's order, on V operands, and every
operation adds U = 2^-24 times the MAGNITUDES of its terms (never their cancelled difference) to what its operands carry -- a
fused multiply-add the compiler forms only removes a rounding.  Anything the expression reads that is itself rounded (the stored
moments, float(1/n), float(bc1)) enters as a V with that rounding as its error.  Where a result has no rounding at all the test
asserts bit equality.  Every bound goes through tolerances.within(measured / bound, 1.0); none is tuned from a run."""
import math
import os
import warnings

import pytest
import torch

import loss_fp64 as R
from fp64_bounds import U, _bits, _f32, _r16, _tag, assert_rounded
from glare_amd import _lib, ops, train_ops
from glare_amd._lib import check, host_f32, ptr, stream_handle
from test_gpu_backward_edges import _block_sum, _ratio, _reduce_depth, _sigmoid_rel, check_f32
from tolerances import within

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = 2.0 ** -149          # the spacing of the fp32 subnormals: what a product or a quotient that underflows can lose
C1, C2 = _f32(0.01 ** 2), _f32(0.03 ** 2)


@pytest.fixture(params=("bf16", "fp16"))
def prec(request):
    with ops.use_precision(request.param):
        yield request.param


def gamma(k):
    """k roundings in a row: (1 + U)^k - 1 <= k U / (1 - k U)"""
    return k * U / (1.0 - k * U)


def _dev(t):
    return t.cuda()


def _t64(x):
    return x if torch.is_tensor(x) else torch.tensor(float(x), dtype=torch.float64, device="cuda")


class V:
    """a quantity the kernel holds in fp32: v = what exact arithmetic gives on the exact operands (fp64), e = a bound on |fp32 - v|.
    Operands that are not V are exact fp32 inputs.  +, -: the operands' errors and one rounding on the sum of the magnitudes;
    *, /: first order and the cross term, one rounding, and TINY for a result in the subnormal range."""

    def __init__(self, v, e=0.0):
        self.v, self.e = _t64(v), _t64(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def mag(self):
        return self.v.abs() + self.e

    def __neg__(self):
        return V(-self.v, self.e)

    def scale(self, k):
        """times a power of two: exact"""
        return V(self.v * k, self.e * abs(k))

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, (self.e + o.e) + U * (self.mag() + o.mag()))

    def __sub__(self, o):
        return self + (-V.of(o))

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e + U * self.mag() * o.mag() + TINY)

    def __truediv__(self, o):
        o = V.of(o)
        lo = o.v.abs() - o.e
        assert bool((lo > 0).all()), "a divisor the bound cannot keep away from 0"
        q = self.v.abs() / o.v.abs()
        return V(self.v / o.v, (self.e + q * o.e) / lo + U * self.mag() / lo + TINY)

    def sqrt(self):
        s = self.v.sqrt()
        hi, lo = (self.v + self.e).sqrt(), (self.v - self.e).clamp_min(0.0).sqrt()
        return V(s, torch.maximum(hi - s, s - lo) + U * hi)


def _same_value(got, want):
    """equal as numbers at every element (+0 and -0 are), and neither side holds a NaN"""
    return bool((got.double() == want.double()).all())


# ---- 1. clamp01 / clamp01_backward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 255, 257, 1000))
def test_clamp01_and_backward_bits(n):
    x = _dev(R.clamp_inputs(n, n))
    y = train_ops.clamp01(x)
    assert y.dtype == torch.float32 and _same_value(y, R.clamp01(x.double()))          # no rounding: the value itself or 0 or 1
    g = torch.randn(n, generator=torch.Generator().manual_seed(n + 1))
    blocked = ~R.clamp01_pass(x.double()).cpu()
    g[blocked] = torch.tensor([math.inf, -math.inf, math.nan])[torch.arange(int(blocked.sum())) % 3]          # must come out +0
    g = _dev(g)
    gx = train_ops.clamp01_backward(x, g)
    want = torch.where(R.clamp01_pass(x.double()), g, torch.zeros_like(g))
    assert torch.equal(_bits(gx), _bits(want))
    if n >= len(R.CLAMP_SPECIALS):          # the closed interval passes, NaN of either sign and one ulp outside do not
        passed = (~blocked[:12]).tolist()
        assert passed == [False, False, False, True, True, True, True, True, False, False, False, False]


# ---- 2. the pixel losses ---------------------------------------------------------------------------------------------------------
def _l1_run(fn, rec, gt):
    B, H, W, C = rec.shape
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    grad = torch.full_like(rec, float("nan"))
    ws = torch.full((512,), float("nan"), dtype=torch.float32, device="cuda")
    check(getattr(_lib.lib(), fn)(ptr(rec), ptr(gt), B, H * W, C, ptr(loss), ptr(grad), ptr(ws), 2048, stream_handle()), fn)
    return loss, grad, ws


def _l1_check(fn, restate, rec32, gt32, tag, finite=True):
    """loss, every gradient element and every per-block partial of one launch"""
    rec, gt = _dev(rec32), _dev(gt32)
    n = rec.numel()
    loss, grad, ws = _l1_run(fn, rec, gt)
    terms, eloss, sign = restate(rec.double(), gt.double())
    # gradient: no rounding beyond float(1 / float(n)) -- sign * that, bit for bit; a NaN (plain form) at the NaN element alone
    inv_n = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    inv_n = inv_n.cuda()
    want = torch.where(sign > 0, inv_n, torch.where(sign < 0, -inv_n, torch.zeros_like(inv_n)))
    nan = torch.isnan(sign)
    assert torch.equal(torch.isnan(grad), nan)
    assert torch.equal(_bits(torch.where(nan, torch.zeros_like(grad), grad)), _bits(want))
    blocks = min(512, -(-n // 1024))
    assert bool(torch.isnan(ws[blocks:]).all())          # the workspace past the last block is untouched
    if not finite:
        return loss
    # partial[blk]: block blk owns the elements i with (i // 256) % blocks == blk (grid-stride loop); a thread adds `trips` terms,
    # each |sr - gt| rounded once; 6 shuffle additions over the wave, 2 over the four waves
    trips = -(-n // (blocks * 256))
    block_of = (torch.arange(n, device="cuda") // 256) % blocks
    pex = _block_sum(terms.reshape(n, 1), block_of, blocks)[:, 0]
    worst = _ratio((ws[:blocks].double() - pex).abs(), gamma(trips + 9) * pex)
    bad = torch.nonzero(worst >= 1).flatten().tolist()
    assert not bad, "%s: partials of blocks %s off by %s x the bound" % (tag, bad[:8], [float(worst[b]) for b in bad[:8]])
    within(float(worst.max()), 1.0, _tag(tag + ":partials"))
    # the loss: the additions of glare_reduce_parts_f32 behind it, the product with inv_n and inv_n's own rounding
    check_f32(loss, eloss.reshape(1), gamma(trips + 9 + _reduce_depth(blocks, 1) + 2) * eloss.reshape(1), tag + ":loss")
    return loss


@pytest.mark.parametrize("shape", R.L1_SHAPES)
def test_l1_clamp_loss_per_element_and_per_block(shape):
    """210 elements: one block; 1053: a sample boundary inside a block; C = 4: the NCHW index of gt; 526 683 > 512 x 1024: some
    threads take a fifth trip.  Every planted special in every sample (one element: each on its own)."""
    tag = "l1_clamp:%dx%dx%dx%d" % shape
    rec, gt = R.l1_inputs(shape, 11)
    n = rec.numel()
    blocks = min(512, -(-n // 1024))
    assert (blocks, -(-n // (blocks * 256))) == {1: (1, 1), 210: (1, 1), 1053: (2, 3), 120: (1, 1), 526683: (512, 5)}[n]          # (blocks, trips)
    if n == 1:
        for name in R.L1_SPECIALS:
            r = rec.clone()
            R.l1_plant(r, gt, 0, 0, name)
            loss = _l1_check("glare_l1_clamp_loss_f32", R.l1_clamp, r, gt, tag + ":" + name)
            assert bool(torch.isfinite(loss).all())
        return
    loss = _l1_check("glare_l1_clamp_loss_f32", R.l1_clamp, rec, gt, tag)
    assert bool(torch.isfinite(loss).all())          # NaN masked, +-inf clamped


@pytest.mark.parametrize("shape", R.L1_SHAPES)
def test_l1_plain_loss_per_element_and_per_block(shape):
    """the finite bound on a draw without NaN / inf; with them the loss is NaN or inf and the gradient NaN at the NaN alone"""
    tag = "l1_plain:%dx%dx%dx%d" % shape
    rec, gt = R.l1_inputs(shape, 11)
    if rec.numel() == 1:
        for name in R.L1_SPECIALS:
            r = rec.clone()
            R.l1_plant(r, gt, 0, 0, name)
            finite = name not in ("pinf", "ninf", "nan")
            loss = _l1_check("glare_l1_loss_f32", R.l1_plain, r, gt, tag + ":" + name, finite)
            assert finite or (bool(torch.isnan(loss)) if name == "nan" else float(loss) == math.inf)
        return
    clean = torch.where(torch.isfinite(rec), rec, torch.full_like(rec, 0.5))
    _l1_check("glare_l1_loss_f32", R.l1_plain, clean, gt, tag)
    assert float(_l1_check("glare_l1_loss_f32", R.l1_plain, torch.where(torch.isnan(rec), torch.full_like(rec, 0.5), rec), gt,
                           tag, False)) == math.inf
    assert bool(torch.isnan(_l1_check("glare_l1_loss_f32", R.l1_plain, rec, gt, tag, False)))


# ---- 3. sigmoid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 257))
def test_sigmoid_per_element(n):
    """1 / (1 + expf(-x)) with the ACCURATE expf (csrc/build.py passes no fast-math flag): no rounding on the way to the exponent,
    so _sigmoid_rel's count with arg_roundings = 0.  Two terms the relative count cannot carry: a result in the subnormal range
    rounds to their spacing (TINY), and for x < -88.72 exp(-x) is past the largest float -- the quotient is 0 and the whole value,
    below 1 / FLT_MAX = 2.9e-39, is the error."""
    planted = [0.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, math.inf, -math.inf, math.nan, 1e-40]
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 6
    if n == 1:
        xs = [torch.tensor([v], dtype=torch.float32) for v in planted]
    else:
        x[:len(planted)] = torch.tensor(planted, dtype=torch.float32)
        xs = [x]
    flt_max = float(torch.finfo(torch.float32).max)
    for x in xs:
        x = _dev(x)
        y = train_ops.sigmoid(x)
        nan = torch.isnan(x)
        assert torch.equal(torch.isnan(y), nan)
        a = torch.where(nan, torch.zeros_like(x), x).double()
        ex, rel = _sigmoid_rel(a, 0)
        lost = torch.where(torch.exp(-a) >= flt_max * (1 - 4 * U), ex, torch.zeros_like(ex))
        check_f32(torch.where(nan, torch.full_like(y, 0.5), y), ex, ex * rel + TINY + lost, "sigmoid:%d" % n)
        assert bool((y[~nan] >= 0).all()) and bool((y[~nan] <= 1).all())


# ---- 4. avgpool2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((1, 2, 2, 1), (1, 3, 2, 3), (2, 5, 7, 3), (1, 64, 66, 3)))
def test_avgpool2_per_element(shape):
    """(2, 5, 7, 3): an odd last row and column are dropped, image 1 is x64 so that a window reaching across the batch boundary or a
    row wrap is far over the bound; (1, 64, 66, 3): 6336 outputs, 25 blocks"""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)))
    if shape[0] > 1:
        x[1] *= 64
    x = _dev(x)
    y = train_ops.avgpool2(x)
    # ((p0 + p1) + p2) + p3: three additions on sum |p|; the scale by 0.25 is exact
    check_f32(y, R.avgpool2(x.double()), gamma(3) * R.avgpool2(x.double().abs()), "avgpool2:%dx%dx%dx%d" % shape)


# ---- 5. SSIM, one level: forward and backward ------------------------------------------------------------------------------------
def _moment_bounds(x, y, w1):
    """[.., 5] bounds of the stored moments: the window product g[dy] * g[dx] rounds once, a * a (a * b) once, then L = ws^2 fma links
    on sum w |term|"""
    L = len(w1) ** 2
    ax, ay = x.abs(), y.abs()
    return torch.stack([gamma(L + 1) * R.windowed(ax, w1), gamma(L + 1) * R.windowed(ay, w1), gamma(L + 2) * R.windowed(ax * ax, w1),
                        gamma(L + 2) * R.windowed(ay * ay, w1), gamma(L + 2) * R.windowed(ax * ay, w1)], -1)


def _ssim_terms(mom, emom):
    """the common subexpressions of ssim_fwd_kernel and ssim_bwd_maps_kernel on the moments AS STORED (exact value, forward bound).
    s1 = e11 - m1 * m1 cancels: the rounding U (e11 + m1^2) stays whole in v2, whose floor is C2 = 9e-4"""
    m1, m2, e11, e22, e12 = (V(mom[..., k], emom[..., k]) for k in range(5))
    s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
    v1, v2 = s12.scale(2.0) + C2, (s1 + s2) + C2
    a1, a2 = m1.scale(2.0) * m2 + C1, (m1 * m1 + m2 * m2) + C1
    return m1, m2, v1, v2, a1, a2


_ssim_cond_rows = {}
SSIM_COND_HEADER = """SSIM (one level, csrc/loss_ops.hip) against the conditioning of its input, measured on an MI355X.
Written by tests/test_gpu_loss_update_edges.py::test_ssim_forward_backward_per_element at B 2, 12 x 17, C 3, the 11-tap window;
every figure is the largest |value - fp64| over the tensor, `bound` the largest per-element bound the test derives for it
(counted from the kernels' expressions: U (E[xx] + mu^2) of the variance's cancellation over v2 >= C2 = 9e-4).
  moments   the five stored windowed moments
  ssim, cs  the two means the forward returns
  gx        the gradient: level 2, all ten upstream values non-zero, with the next level's gradient added

family          moments       bound          ssim       bound            cs       bound            gx       bound
"""


@pytest.mark.parametrize("family", R.SSIM_FAMILIES)
@pytest.mark.parametrize("shape", R.SSIM_SHAPES)
def test_ssim_forward_backward_per_element(shape, family):
    """(1, 11, 11, 3, 11): one output pixel; (2, 12, 17, 3, 11): ragged, two images; windows of 5, 3 and 1 taps; (1, 158, 158, 3, 11):
    65 712 outputs > 256 x 256, the forward's grid-stride loop takes a second trip.  The backward runs through the C ABI with the
    test's own scratch buffer: level 0 with g_sim[0] = 0 (how MS-SSIM uses levels 0-3) and the next level's gradient, level 2 with
    everything non-zero, level 4 without a next level.  With odd H or W the last row / column receives no g_next.
    The backward's reference differentiates the EXACT moments; the kernel reads the stored fp32 ones, whose forward bound is
    propagated through -- through 1 / v2, about a 1 / C2 = 1.1e3 amplification (twice in d / d E[xx]), which is why these bounds are
    loose on the bright and flat families: see profiles/ssim_conditioning.txt."""
    B, H, W, C, ws = shape
    tag = "ssim:%dx%dx%dx%d:%s" % (B, H, W, C, family)
    x32, y32 = R.ssim_inputs(shape, family, H * 100 + W)
    x, y = _dev(x32), _dev(y32)
    w1 = R.gaussian_window(ws)
    assert ws == min(11, H, W)
    OH, OW = H - ws + 1, W - ws + 1
    n = B * OH * OW * C
    assert (n > 65536) == (H == 158)
    mom, out = train_ops.ssim_forward(x, y, w1, C1, C2)
    xd, yd = x.double(), y.double()
    emom, esim, ecs = R.ssim_forward(xd, yd, w1, C1, C2)
    bmom = _moment_bounds(xd, yd, w1)
    check_f32(mom, emom, bmom, tag + ":moments")
    # the two means: per pixel the kernel's expression on the stored moments; block sums in double; one rounding to float
    m1, m2, v1, v2, a1, a2 = _ssim_terms(emom, bmom)
    cs, ss = v1 / v2, (a1 * v1) / (a2 * v2)
    bsim, bcs = (p.e.mean() + U * p.v.mean().abs() + 1e-13 for p in (ss, cs))
    assert abs(float(ss.v.mean() - esim)) < 1e-11 and abs(float(cs.v.mean() - ecs)) < 1e-11
    check_f32(out, torch.stack([esim, ecs]), torch.stack([bsim, bcs]), tag + ":means")
    row = None
    lib = _lib.lib()
    for level, zero_sim, with_next in ((0, True, True), (2, False, True), (4, False, False)):
        g10 = torch.tensor([0.7, -0.4, 0.9, 1.3, -0.6, 0.5, -1.1, 0.8, -0.3, 1.2], dtype=torch.float32)
        if zero_sim:
            g10[level] = 0.0
        g_next = None
        if with_next:
            g_next = _dev(torch.randn(B, H // 2, W // 2, C, generator=torch.Generator().manual_seed(level)) * 1e-3)
        g10 = _dev(g10)
        scratch = torch.full((B, OH, OW, C, 3), float("nan"), dtype=torch.float32, device="cuda")
        gx = torch.full_like(x, float("nan"))
        check(lib.glare_ssim_backward_f32(ptr(x), ptr(y), ptr(mom), B, H, W, C, host_f32(w1), ws, C1, C2, ptr(g10), level,
                                          ptr(g_next) if g_next is not None and g_next.numel() else None, ptr(scratch), ptr(gx),
                                          stream_handle()), "glare_ssim_backward_f32")
        g_sim, g_cs = float(g10[level]), float(g10[5 + level])
        eadj = R.ssim_adjoints(emom, C1, C2, g_sim, g_cs)
        # ssim_bwd_maps_kernel, in its order
        alpha, beta = V(g_sim) / float(n), V(g_cs) / float(n)
        cs, lum, iv2, ia2 = v1 / v2, a1 / a2, V(1.0) / v2, V(1.0) / a2
        dcs_m1 = (m2.scale(-2.0) - cs * m1.scale(-2.0)) * iv2
        dcs_e11 = (-cs) * iv2
        dcs_e12 = iv2.scale(2.0)
        dl_m1 = (m2.scale(2.0) - lum.scale(2.0) * m1) * ia2
        w_cs = alpha * lum + beta
        o = [alpha * dl_m1 * cs + w_cs * dcs_m1, w_cs * dcs_e11, w_cs * dcs_e12]
        ov = torch.stack([p.v for p in o], -1)
        assert bool(((ov - eadj).abs() <= 1e-4 * torch.stack([p.e for p in o], -1)).all())          # the same function, fp64 apart
        ltag = "%s:l%d" % (tag, level)
        check_f32(scratch, eadj, torch.stack([p.e for p in o], -1), ltag + ":adjoints")
        # ssim_bwd_gather_kernel: at most ws^2 fma links (and the rounded window product) on sum w |o|, the maps' own errors
        # gathered; r = (a0 + (2 x) a1) + y a2, then + 0.25 g_next (the scale exact)
        acc = [V(R.windowed_adjoint(p.v, w1, H, W),
                 R.windowed_adjoint(p.e, w1, H, W) + gamma(ws * ws + 1) * R.windowed_adjoint(p.mag(), w1, H, W)) for p in o]
        r = (acc[0] + V(xd).scale(2.0) * acc[1]) + V(yd) * acc[2]
        if with_next and g_next.numel():
            up = torch.zeros_like(xd)
            up[:, :H // 2 * 2, :W // 2 * 2] = 0.25 * g_next.double().repeat_interleave(2, 1).repeat_interleave(2, 2)
            has = torch.zeros_like(xd, dtype=torch.bool)
            has[:, :H // 2 * 2, :W // 2 * 2] = True
            rn = r + V(up)
            r = V(torch.where(has, rn.v, r.v), torch.where(has, rn.e, r.e))
        egx = R.ssim_backward(xd, yd, eadj, w1, g_next.double() if with_next else None)
        assert bool(((r.v - egx).abs() <= 1e-4 * r.e).all())
        check_f32(gx, egx, r.e, ltag + ":gx")
        if level == 2:
            row = (float((gx.double() - egx).abs().max()), float(r.e.max()))
    if shape == (2, 12, 17, 3, 11):
        _ssim_cond_rows[family] = ("%-12s %10.3e  %10.3e    %10.3e  %10.3e    %10.3e  %10.3e    %10.3e  %10.3e\n"
                                   % (family, float((mom.double() - emom).abs().max()), float(bmom.max()),
                                      abs(float(out[0]) - float(esim)), float(bsim), abs(float(out[1]) - float(ecs)), float(bcs), row[0], row[1]))
        outdir = os.path.join(ROOT, os.environ.get("GLARE_OUT_DIR", "out"))
        try:
            os.makedirs(outdir, exist_ok=True)
            with open(os.path.join(outdir, "ssim_conditioning.txt"), "w") as f:
                f.write(SSIM_COND_HEADER + "".join(_ssim_cond_rows[k] for k in R.SSIM_FAMILIES if k in _ssim_cond_rows))
        except OSError as e:       # a read-only tree: the checks above have run, only the table is lost -- say so
            warnings.warn("ssim_conditioning.txt not written: %s" % e)


# ---- 6. maxpool2 / maxpool2_backward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES)
def test_maxpool2_and_backward_bits(prec, shape):
    """values from {-2, -1, -0.0, 0.0, 1, 2, +-inf, the largest finite}: every one a 16-bit number, so neither pass rounds.  More than
    half the windows tie for the maximum (test_loss_fp64_host.py asserts it of these inputs): the gradient goes to the FIRST maximum
    in scan order, +0 to everyone else and to the odd last row / column of (1, 3, 2, 8) and (2, 5, 7, 3)."""
    B, H, W, C = shape
    big = float(torch.finfo(ops.act_dtype()).max)
    x32 = R.maxpool_inputs(shape, big, 5)
    x = _dev(_r16(x32))
    assert torch.equal(x.float().cpu(), x32)
    y = train_ops.maxpool2(x)
    assert y.dtype == ops.act_dtype() and y.shape == (B, H // 2, W // 2, C)
    assert _same_value(y, R.maxpool2(x.double()))
    g = _dev(_r16(torch.randn(B, H // 2, W // 2, C, generator=torch.Generator().manual_seed(6)) + 3.0))          # no zero among them
    assert bool((g != 0).all())
    gx = torch.full_like(x, float("nan"))
    check(_lib.lib().glare_maxpool2_backward_bf16(ptr(x), ptr(g), ptr(gx), B, H, W, C, stream_handle()), "glare_maxpool2_backward_bf16")
    want = R.maxpool2_backward(x.double(), g.double())
    assert torch.equal(_bits(gx), _bits(want.to(ops.act_dtype())))          # a copy of g, or +0: bit for bit
    assert int((gx != 0).sum()) == g.numel()          # exactly one receiver per window


# ---- 7. feature MSE --------------------------------------------------------------------------------------------------------------
def _mse_operands(n):
    g = torch.Generator().manual_seed(n)
    a, b = _r16(torch.randn(n, generator=g)), _r16(torch.randn(n, generator=g))
    if n > 4:
        b[1] = a[1]          # an exact zero difference
        a[2], b[2] = 30.0, -30.0
    return _dev(a), _dev(b)


@pytest.mark.parametrize("n", (1, 255, 257, 4099, 65537))
def test_mse_loss_per_element(prec, n):
    """65 537 elements = 257 blocks of work on a grid capped at 256: block 0 takes a second trip.  With and without grad_a."""
    a, b = _mse_operands(n)
    ad, bd = a.double(), b.double()
    eloss = R.mse(ad, bd).reshape(1)
    for want_grad in (False, True):
        loss, ga = train_ops.mse_loss(a, b, want_grad)
        # d = a - b rounds once, d * d once; the sums and the division by n are double (2^-53 per addition); the cast to float once
        check_f32(loss, eloss, (gamma(3) + n * 2.0 ** -52) * eloss + TINY, "mse:%d:loss:%d" % (n, want_grad))
        if want_grad:
            # round16(2 d inv_n): d once, float(1 / n) once, the product once (2 d is exact)
            eg = R.mse_backward(ad, bd, 1.0)
            assert_rounded(ga, eg, gamma(3) * eg.abs() + TINY, "mse:%d:grad_a" % n)
        else:
            assert ga is None


@pytest.mark.parametrize("n", (1, 255, 257, 4099, 65537, 524293))
def test_mse_backward_per_element(prec, n):
    """524 293 elements = 2049 blocks of work on a grid capped at 2048.  g = 1 at n = 65 537 puts 2 d / n in fp16's subnormal range
    (ulp16 handles it); g = 65536 is the loss scale it is multiplied by BEFORE the 16-bit rounding; g = 0 must give exact zeros."""
    a, b = _mse_operands(n)
    ad, bd = a.double(), b.double()
    for gv in (1.0, 65536.0, -3.5, 0.0):
        g = torch.tensor([gv], dtype=torch.float32, device="cuda")
        ga = train_ops.mse_backward(a, b, g)
        eg = R.mse_backward(ad, bd, gv)
        # s = (2 inv_n) g: float(1 / n) and the product; (a - b) s: the difference and the product
        assert_rounded(ga, eg, gamma(4) * eg.abs() + TINY, "mse_bwd:%d:%g" % (n, gv))
        if gv == 0.0:
            assert int(_bits(ga).abs().max() & 0x7fff) == 0


# ---- 8. Adam ---------------------------------------------------------------------------------------------------------------------
LR, EPS = 2e-4, 1e-8
#             entry      betas          step  wd    grad_scale  loss_scale  lr multiplier
ADAM_CONFIGS = (("host", (0.9, 0.999), 1, 0.0, 1.0, None, 1.0),
                ("host", (0.5, 0.9), 2, 0.01, 0.5, None, 1.0),
                ("host", (0.9, 0.999), 1000, 0.0, 1.0 / 3, None, 1.0),
                ("dev", (0.9, 0.999), 10, 0.01, 1.0, None, 0.25),
                ("dev", (0.5, 0.9), 1, 0.0, 1.0 / 3, None, 1.0),
                ("dev", (0.9, 0.999), 1000, 0.0, 1.0, None, 1.0),
                ("guarded", (0.9, 0.999), 2, 0.0, 0.5, None, 1.0),
                ("guarded", (0.5, 0.9), 1000, 0.01, 1.0, None, 0.25),
                ("scaled", (0.9, 0.999), 1, 0.0, 1.0, 65536.0, 1.0),
                ("scaled", (0.5, 0.9), 10, 0.01, 0.5, 3.0, 0.25),
                ("scaled", (0.9, 0.999), 1000, 0.0, 1.0 / 3, 3.0, 1.0),
                ("scaled", (0.5, 0.9), 2, 0.0, 1.0, 65536.0, 1.0))
GRAD_FAMILIES = (("normal", 1.0), ("near_eps", 1e-8), ("underflow", 1e-23), ("huge", 1e18), ("zero", 0.0))


def _adam_state(n, t, betas, lr_mul):
    """step_dev = t - 1 and a state3 whose bias entries are junk: adam_prepare must write them"""
    step_dev = torch.tensor([t - 1], dtype=torch.int32, device="cuda")
    state3 = torch.tensor([7.0, 7.0, lr_mul], dtype=torch.float32, device="cuda")
    return step_dev, state3


def _adam_launch(entry, w, g, m, v, t, betas, wd, gs, ls, lr_mul, skip_value=0):
    """one optimizer step through `entry`; -> (step_dev, state3) or None for the host entry point"""
    if entry == "host":
        train_ops.adam_step_(w, g, m, v, t, LR, betas, EPS, wd, gs)
        return None
    step_dev, state3 = _adam_state(w.numel(), t, betas, lr_mul)
    if entry == "dev":
        train_ops.adam_prepare_(step_dev, state3, betas)
        train_ops.adam_step_dev_(w, g, m, v, state3, LR, betas, EPS, wd, gs)
        return step_dev, state3
    skip = torch.tensor([skip_value], dtype=torch.int32, device="cuda")
    train_ops.adam_prepare_guarded_(step_dev, state3, betas, skip)
    loss_scale = torch.tensor([ls], dtype=torch.float32, device="cuda") if entry == "scaled" else None
    train_ops.adam_step_dev_guarded_(w, g, m, v, state3, LR, betas, EPS, wd, gs, skip, loss_scale)
    return step_dev, state3


def _adam_bound(entry, w, g, m, v, t, betas, wd, gs, ls, lr_mul):
    """adam_kernel's expression on V operands; the scalars as the C floats the ABI receives.  bc1 = 1 - b1^t and sqrt(1 - b2^t) are
    formed in double and rounded to float once (pow's own error, 1e-16, is carried as well)."""
    b1, b2, lr, eps, wdf, gsf = (_f32(s) for s in (betas[0], betas[1], LR, EPS, wd, gs))
    bc1, bc2s = R.adam_bias(b1, b2, t)
    bc1, bc2s = V(bc1, U * bc1 + 1e-15), V(bc2s, U * bc2s + 1e-14)
    lrv = V(lr) * _f32(lr_mul) if entry != "host" else V(lr)
    scale = V(gsf) / _f32(ls) if ls is not None else V(gsf)
    gi = V(g) * scale
    if wd != 0.0:
        gi = gi + V(wdf) * w
    mi = V(b1) * m + (V(1.0) - b1) * gi
    vi = V(b2) * v + (V(1.0) - b2) * gi * gi
    denom = vi.sqrt() / bc2s + eps
    return V(w) - (lrv / bc1) * (mi / denom), mi, vi, (b1, b2, lr, eps, wdf, gsf)


@pytest.mark.parametrize("cfg", ADAM_CONFIGS, ids=lambda c: "%s-b%g-t%d-wd%g-gs%.2g-ls%s-mul%g" % (c[0], c[1][0], c[2], c[3], c[4], c[5], c[6]))
def test_adam_per_element(cfg):
    """n = 255, 256, 257: one short of a block, a full one, one over.  From w = m = v = 0 the final subtraction is exact and the update
    is seen at its own precision instead of hiding under U |w|; then from a random state with v >= 0.  Gradients N(0, 1), at 1e-8
    (sqrt(v) beside eps), at 1e-23 (g^2 underflows), at 1e18, and exact zeros (with m = v = 0 and no decay: w bit-unchanged)."""
    entry, betas, t, wd, gs, ls, lr_mul = cfg
    for n in (1, 255, 256, 257, 1000):
        for zero_state in (True, False):
            for fam, gscale in GRAD_FAMILIES:
                gen = torch.Generator().manual_seed(n * 7 + t)
                g0 = _dev(torch.randn(n, generator=gen) * gscale)
                if zero_state:
                    w0, m0, v0 = (torch.zeros(n, device="cuda") for _ in range(3))
                else:
                    w0 = _dev(torch.randn(n, generator=gen))
                    m0 = _dev(torch.randn(n, generator=gen) * max(gscale, 1e-30) * 0.1)
                    v0 = _dev((torch.randn(n, generator=gen) * max(gscale, 1e-30)) ** 2 * 0.01)
                w, m, v = w0.clone(), m0.clone(), v0.clone()
                st = _adam_launch(entry, w, g0, m, v, t, betas, wd, gs, ls, lr_mul)
                bw, bm, bv, (b1, b2, lr, eps, wdf, gsf) = _adam_bound(entry, w0.double(), g0.double(), m0.double(), v0.double(), t, betas,
                                                                       wd, gs, ls, lr_mul)
                ew, em, ev = R.adam_step(w0.double(), g0.double(), m0.double(), v0.double(), lr, b1, b2, eps, wdf, t, gsf,
                                         _f32(ls) if ls is not None else None, _f32(lr_mul) if entry != "host" else 1.0)
                tag = "adam:%s:%s:%d" % (entry, fam, zero_state)
                check_f32(m, em, bm.e, tag + ":m")
                check_f32(v, ev, bv.e, tag + ":v")
                check_f32(w, ew, bw.e, tag + ":w")
                assert bool(torch.isfinite(v).all()) and bool((v >= 0).all())
                if fam == "zero" and zero_state and wd == 0.0:
                    assert torch.equal(_bits(w), _bits(w0)) and int(_bits(m).abs().max()) == 0 and int(_bits(v).abs().max()) == 0
                elif fam != "zero":
                    assert not torch.equal(_bits(m), _bits(m0))
                if st is not None:
                    assert int(st[0]) == t and float(st[1][2]) == _f32(lr_mul)


@pytest.mark.parametrize("entry", ("guarded", "scaled"))
def test_adam_skip_flag_freezes_everything(entry):
    """a non-zero skip flag (GradScaler found inf / NaN): w, m, v, step_dev and state3 bit-identical through prepare AND step;
    with a zero flag they move"""
    n, t, betas = 257, 10, (0.5, 0.9)
    gen = torch.Generator().manual_seed(3)
    w0, g0, m0 = (_dev(torch.randn(n, generator=gen)) for _ in range(3))
    v0 = _dev(torch.rand(n, generator=gen))
    g0[5] = math.inf
    for skip_value in (1, -7, 0):
        w, m, v = w0.clone(), m0.clone(), v0.clone()
        step_dev, state3 = _adam_launch(entry, w, g0, m, v, t, betas, 0.01, 1.0, 65536.0, 0.25, skip_value)
        frozen = all(torch.equal(_bits(a), _bits(b)) for a, b in ((w, w0), (m, m0), (v, v0)))
        same_state = int(step_dev) == t - 1 and torch.equal(_bits(state3), _bits(_adam_state(n, t, betas, 0.25)[1]))
        if skip_value:
            assert frozen and same_state, skip_value
        else:
            moved = [not torch.equal(_bits(a), _bits(b)) for a, b in ((w, w0), (m, m0), (v, v0))]
            assert all(moved) and int(step_dev) == t and float(state3[0]) != 7.0 and float(state3[1]) != 7.0


@pytest.mark.parametrize("betas", ((0.9, 0.999), (0.5, 0.9)))
@pytest.mark.parametrize("t", (1, 2, 10, 1000, 100000))
def test_adam_prepare(betas, t):
    """step_dev: t - 1 -> t; state3[0:2] = (1 - b1^t, sqrt(1 - b2^t)) formed in double (pow and sqrt of a double: 1e-16 relative, through
    the sqrt at most 1e-14 absolute) and rounded to float ONCE; state3[2], the lr multiplier, untouched"""
    for guarded in (False, True):
        step_dev, state3 = _adam_state(1, t, betas, 0.25)
        if guarded:
            train_ops.adam_prepare_guarded_(step_dev, state3, betas, torch.zeros(1, dtype=torch.int32, device="cuda"))
        else:
            train_ops.adam_prepare_(step_dev, state3, betas)
        assert int(step_dev) == t
        bc1, bc2s = R.adam_bias(_f32(betas[0]), _f32(betas[1]), t)
        within(abs(float(state3[0]) - bc1) / (U * bc1 + 1e-15), 1.0, "adam_prepare:bc1")
        within(abs(float(state3[1]) - bc2s) / (U * bc2s + 1e-14), 1.0, "adam_prepare:bc2_sqrt")
        assert float(state3[2]) == 0.25


# ---- 9. grad_nonfinite -----------------------------------------------------------------------------------------------------------
NONFINITE = (0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001)          # +inf, -inf, a quiet NaN, a negative NaN, 0x7f800001
CLEAN = (0x7f7fffff, 0xff7fffff, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00000000, 0x80000000, 0x3f800000, 0xc2280000)


def _i32(bits):
    return bits - (1 << 32) if bits >= 1 << 31 else bits


@pytest.mark.parametrize("n", (1, 255, 256, 257, 4096, 4097, 8193, 4096 * 4096 + 257))
def test_grad_nonfinite(n):
    """a thread reads 16 elements of a block's 4096; the grid is capped at 4096 blocks, so 4096 * 4096 + 257 elements is the first
    size with a 17th trip.  One non-finite value at a time: the first element, the last, the first of the last trip.  The largest
    finite value, subnormals and +-0 are clean; `found` is only ever ORed into."""
    for b in NONFINITE + CLEAN:
        assert R.nonfinite_bits(b) == (b in NONFINITE)
    clean = torch.tensor([_i32(b) for b in CLEAN], dtype=torch.int32, device="cuda")
    buf = clean[torch.arange(n, device="cuda") % len(CLEAN)].contiguous()
    grad = buf.view(torch.float32)
    blocks = min(4096, -(-n // 4096))
    stride = blocks * 256
    trips = -(-n // stride)
    assert (trips == 17) == (n > 4096 * 4096) and trips <= 17
    for start in (0, 1, 4):
        found = torch.tensor([start], dtype=torch.int32, device="cuda")
        train_ops.grad_nonfinite_(grad, found)
        assert int(found) == start, "a clean buffer changed found %d -> %d" % (start, int(found))
    for pos in sorted({0, n - 1, (trips - 1) * stride}):
        keep = int(buf[pos])
        for bits in NONFINITE:
            buf[pos] = _i32(bits)
            for start in (0, 4):
                found = torch.tensor([start], dtype=torch.int32, device="cuda")
                train_ops.grad_nonfinite_(grad, found)
                assert int(found) == start | 1, "n %d: %#x at %d not found" % (n, bits, pos)
        buf[pos] = keep
    found = torch.zeros(1, dtype=torch.int32, device="cuda")
    train_ops.grad_nonfinite_(grad, found)
    assert int(found) == 0


# ---- 10. gradscaler_update -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", R.SCALER_TABLE, ids=lambda r: "s%g-t%d-f%d-g%g-b%g-i%d" % r)
def test_gradscaler_update_table(row):
    """bit for bit against the restatement of ATen's _amp_update_scale_ (test_loss_fp64_host.py holds it to ATen itself): the scale
    that would grow to inf is KEPT and the tracker reset"""
    scale, tracker, found, growth, backoff, interval = row
    s = torch.tensor([scale], dtype=torch.float32, device="cuda")
    t = torch.tensor([tracker], dtype=torch.int32, device="cuda")
    f = torch.tensor([found], dtype=torch.int32, device="cuda")
    train_ops.gradscaler_update_(s, t, f, growth, backoff, interval)
    es, et = R.scaler_update(scale, tracker, found, growth, backoff, interval)
    got = int(_bits(s)[0]) & 0xffffffff
    assert (got, int(t)) == (R.f32_bits(es), et), "scale %g (%#x), tracker %d; expected %g (%#x), %d" % (
        float(s), got, int(t), float(es), R.f32_bits(es), et)
    assert int(f) == found          # the flag is the caller's to clear
