"""GPU: the HBM-bound streaming kernels (csrc/elementwise.hip, gn.hip, flow.hip) PER ELEMENT against fp64 restatements of the
same operation, at the shapes where their index arithmetic can go wrong: more than one block per image with a ragged last block,
pitch / offset inside wider records, the second trip of a grid-stride loop, tiles that straddle C or HW, every unroll remainder.

Every kernel here rounds once, on its 16-bit store (or not at all: the fp32 flow state), so the bound is derived, not measured:
    |got - exact| <= 0.5 ulp16(exact) + slack
with `slack` the fp32 evaluation error of the kernel's own expression, counted from its source and stated next to each call
(U = 2^-24, the relative error of ONE fp32 rounding).  The operands are rounded to the 16-bit format before either side sees them.
Every bound goes through tolerances.within(measured / bound, 1.0), whose table of measured values lists how much of it is used."""
import math
import os
import warnings

import pytest
import torch
import torch.nn.functional as F

from glare_amd import _lib, ops, train_ops
from glare_amd._lib import check, ptr, stream_handle
from fp64_bounds import U, _bits, _f32, _fmt, _r16, _tag, assert_f32, assert_rounded, ulp16
from tolerances import within

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=("bf16", "fp16"))
def prec(request):
    with ops.use_precision(request.param):
        yield request.param


# ---- shared helpers (plain torch, fp64) -------------------------------------------------------------------------------------------
def assert_pair(hi, lo, exact64, slack64, tag):
    """a hi / lo pair: the remainder half is rounded once more, at the ulp of `lo` (|lo| <= 0.5 ulp16(exact))"""
    assert hi.dtype == lo.dtype == ops.act_dtype() and hi.shape == lo.shape == exact64.shape
    err = (hi.double() + lo.double() - exact64).abs()
    return within(float((err / (0.5 * ulp16(0.5 * ulp16(exact64)) + slack64)).max()), 1.0, _tag(tag))


def _terms(per):
    """fp32 additions behind one block partial of the two-level sums: 8 elements per 16-B vector, ceil(per / 256) vectors per thread,
    6 wave shuffles, 3 adds across the four waves"""
    return 8 * -(-per // 256) + 9


def _block_sums(v64, bps):
    """[B, n] fp64 -> (sum, sum of magnitudes) over exactly the slices [blk * per, min(nvec, (blk + 1) * per)) of 8-element vectors"""
    B, n = v64.shape
    nvec = n // 8
    per = -(-nvec // bps)
    s = torch.stack([v64[:, blk * per * 8:min(nvec, (blk + 1) * per) * 8].sum(1) for blk in range(bps)], 1)
    a = torch.stack([v64[:, blk * per * 8:min(nvec, (blk + 1) * per) * 8].abs().sum(1) for blk in range(bps)], 1)
    return s, a, per


# ---- 1. mix -----------------------------------------------------------------------------------------------------------------------
MIX_W = (-0.6, 0.3, 5.0)
RESCALE_N = (8, 32768 + 8, 3 * 16384 + 8)          # blocks per sample 1, 2, 3; the last block ragged in the latter two


@pytest.fixture(scope="module")
def mix_big():
    """the grid-stride case, built once per precision and released with the module: 4099 pixels x 2048 channels = 1 049 344 chunks
    > 4096 x 256"""
    cache = {}

    def get():
        key = ops.precision()
        if key not in cache:
            g = torch.Generator().manual_seed(11)
            cache[key] = tuple(_r16(torch.randn(4099, 2048, generator=g)).cuda() for _ in range(2))
        return cache[key]

    yield get
    cache.clear()


def _mix_exact(a, b, w):
    """exact = a f + b (1 - f), f = sigmoid(w) of the fp32 logit the kernel receives.
    slack 8 U (|a| + |b|): f from expf and a division (a few ulp of f), 1 - f inherits f's ABSOLUTE error (so the slack is on
    |a| + |b|, not on |a| f + |b| (1 - f)), two products and a sum"""
    f = 1.0 / (1.0 + math.exp(-_f32(w)))
    a64, b64 = a.double(), b.double()
    return a64 * f + b64 * (1.0 - f), 8 * U * (a64.abs() + b64.abs())


def _logit(w, form):
    return torch.tensor(w, dtype=torch.float32, device="cuda") if form == "dev" else w


@pytest.mark.parametrize("form", ("host", "dev"))
@pytest.mark.parametrize("w", MIX_W)
def test_mix_per_element(prec, mix_big, w, form):
    g = torch.Generator().manual_seed(1)
    wl = _logit(w, form)
    # one chunk
    a, b = (_r16(torch.randn(1, 8, generator=g)).cuda() for _ in range(2))
    exact, slack = _mix_exact(a, b, w)
    assert_rounded(ops.mix(a, b, wl), exact, slack, "mix:1x8:%s:%g" % (form, w))
    # 8 channels inside wider records
    a, b = _r16(torch.randn(5, 24, generator=g)).cuda(), _r16(torch.randn(5, 16, generator=g)).cuda()
    out = torch.full((5, 32), -7.0, dtype=ops.act_dtype(), device="cuda")
    before = out.clone()
    ops.mix(a, b, wl, out=out, out_off=16, a_off=8, b_off=8, C=8)
    exact, slack = _mix_exact(a[:, 8:16], b[:, 8:16], w)
    assert_rounded(out[:, 16:24], exact, slack, "mix:pitched:%s:%g" % (form, w))
    assert torch.equal(out[:, :16], before[:, :16]) and torch.equal(out[:, 24:], before[:, 24:])
    # the second trip of the grid-stride loop
    a, b = mix_big()
    exact, slack = _mix_exact(a, b, w)
    assert_rounded(ops.mix(a, b, wl), exact, slack, "mix:4099x2048:%s:%g" % (form, w))


@pytest.mark.parametrize("form", ("host", "dev"))
@pytest.mark.parametrize("w", MIX_W)
def test_mix_with_sums_per_element_and_per_block(prec, w, form):
    g = torch.Generator().manual_seed(2)
    B = 3
    for n, want_bps in zip(RESCALE_N, (1, 2, 3)):
        a, b = (_r16(torch.randn(B, n, generator=g) + 0.2).cuda() for _ in range(2))
        out, sums = ops.mix_with_sums(a, b, _logit(w, form))
        bps = sums.numel() // B
        assert bps == want_bps
        exact, slack = _mix_exact(a, b, w)
        assert_rounded(out, exact, slack, "mix_sum:%d:%s:%g" % (n, form, w))
        # each partial is the sum of the STORED outputs of exactly its slice; fp32 summation of _terms(per) additions per chain
        s, mag, per = _block_sums(out.double(), bps)
        within(float(((sums.view(B, bps).double() - s).abs() / (_terms(per) * U * mag)).max()), 1.0,
               _tag("mix_sum_partials:%d:%s:%g" % (n, form, w)))


# ---- 2. mean rescale --------------------------------------------------------------------------------------------------------------
def _cond(v64, whole):
    """sum |x| / |sum x| per image (or of the whole batch), [B]"""
    if whole:
        return (v64.abs().sum() / v64.sum().abs()).expand(v64.shape[0])
    return v64.abs().sum(1) / v64.sum(1).abs()


def _ratio64(h64, x64, whole):
    if whole:
        return (h64.sum() / x64.sum()).expand(h64.shape[0])
    return h64.sum(1) / x64.sum(1)


def _rescale_inputs(n, seed):
    """h ~ N(0.2 + 0.1 b, 1), xw ~ N(0.3 + 0.2 b, 1): per-image means that differ clearly and stay away from zero"""
    g = torch.Generator().manual_seed(seed)
    h = torch.stack([torch.randn(n, generator=g) + 0.2 + 0.1 * b for b in range(3)])
    xw = torch.stack([torch.randn(n, generator=g) + 0.3 + 0.2 * b for b in range(3)])
    return h, xw


# seeds at which the 8-element images keep sum|x| / |sum x| < 5 (the larger sizes do so at any seed)
RESCALE_SEED = {8: 7, 32768 + 8: 1, 3 * 16384 + 8: 2}


def _check_rescale_output(out, h, xw, whole, per, tag):
    """ratio bound (relative, from the two fp32 sums: _terms(per) additions each, 8 for the tile / partial roundings, the fp32 ratio
    and its product) and the output: exact = h + xw r64; slack = the fp32 h + xw * r (2 roundings) + |xw| * the ratio's bound"""
    h64, x64 = h.double().flatten(1), xw.double().flatten(1)
    ch, cx = _cond(h64, whole), _cond(x64, whole)
    assert float(ch.max()) < 5 and float(cx.max()) < 5, (ch, cx)         # the inputs are as conditioned as the case asks
    r64 = _ratio64(h64, x64, whole)
    rb = (_terms(per) + 8) * U * (ch + cx) * r64.abs().clamp_max(1.0)
    exact = h64 + x64 * r64[:, None]
    slack = 4 * U * (h64.abs() + (x64 * r64[:, None]).abs()) + x64.abs() * rb[:, None]
    assert_rounded(out.flatten(1), exact, slack, tag)
    return r64, rb


@pytest.mark.parametrize("n", RESCALE_N)
@pytest.mark.parametrize("whole", (False, True))
def test_mean_rescale_per_block_and_per_element(prec, whole, n):
    """The kernel's ratio is taken from its own workspace (the per-block fp32 partials, combined as the apply pass combines them)
    instead of being read back as (out - h) / xw: `out` is a 16-bit tensor, so that quotient carries 0.5 ulp16(out) / |xw|, two
    orders above the ratio's bound in bf16.  The bound and the fp64 reference are the ones of the ratio check.
    What the ':ratio' record is NOT: a measurement of rescale_apply_kernel.  That kernel keeps its ratio in LDS; the record is this
    test's fp64 recombination of partials it has just checked block by block.  The apply kernel's own combine over b0..b1 is pinned
    through the 16-bit output only (0.5 ulp16 + the ratio's bound times |xw|): enough to catch a wrong image or whole-batch selection,
    not a last-bit difference of the ratio.  The fused form (next test) does check the ratio the kernel wrote."""
    B = 3
    hc, xc = _rescale_inputs(n, RESCALE_SEED[n])
    h, xw = _r16(hc).cuda(), xc.cuda()
    lib = _lib.lib()
    nbytes = int(lib.glare_mean_rescale_workspace_bytes(B, n))
    bps = nbytes // (B * 2 * 4)
    assert bps == {8: 1, 32768 + 8: 2, 3 * 16384 + 8: 3}[n]

    def run(xw_):
        ws = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
        out = torch.full_like(h, float("nan"))
        check(lib.glare_mean_rescale_bf16(ptr(h), ptr(xw_), ptr(out), B, n, int(whole), ptr(ws), nbytes, stream_handle()),
              "glare_mean_rescale_bf16")
        return out, ws.view(B, bps, 2).double()

    out, part = run(xw)
    assert torch.equal(_bits(out), _bits(ops.mean_rescale(h, xw, whole_batch=whole)))
    tag = "rescale:%d:%d" % (n, whole)
    for k, v in ((0, h.double()), (1, xw.double())):
        s, mag, per = _block_sums(v, bps)
        within(float(((part[..., k] - s).abs() / (_terms(per) * U * mag)).max()), 1.0, _tag(tag + ":partials%d" % k))
    r64, rb = _check_rescale_output(out, h, xw, whole, per, tag + ":out")
    sh, sx = part[..., 0].sum(1), part[..., 1].sum(1)
    rk = ((sh.sum() / sx.sum()).expand(B) if whole else sh / sx).float().double()        # the apply pass's combine, redone here
    within(float(((rk - r64).abs() / rb).max()), 1.0, _tag(tag + ":ratio"))
    if not whole:      # an image's ratio comes from its own partials only
        xw3 = xw.clone()
        xw3[1] *= 3
        out3, _ = run(xw3)
        assert torch.equal(_bits(out3[0]), _bits(out[0])) and torch.equal(_bits(out3[2]), _bits(out[2]))


def _tile_sums(xw, tile_pixels):
    """what the producer of xw hands over: fp32 sums of its values per tile of pixels, tiles cut per image (the last one ragged)"""
    B, pix, _ = xw.shape
    tiles = -(-pix // tile_pixels)
    pp = F.pad(xw.double().sum(2), (0, tiles * tile_pixels - pix))
    return pp.view(B, tiles, tile_pixels).sum(2).float().contiguous()


@pytest.mark.parametrize("n", RESCALE_N)
@pytest.mark.parametrize("x16", (False, True))
@pytest.mark.parametrize("whole", (False, True))
def test_mean_rescale_fused_per_element(prec, whole, x16, n):
    B, C = 3, 8
    pix = n // C
    ac, xc = _rescale_inputs(n, RESCALE_SEED[n])
    bc, _ = _rescale_inputs(n, RESCALE_SEED[n] + 100)
    h, hs = ops.mix_with_sums(_r16(ac).cuda().view(B, pix, C), _r16(bc).cuda().view(B, pix, C), 0.3)
    bps = hs.numel() // B
    per = -(-(n // 8) // bps)
    xw = (_r16(xc) if x16 else xc).cuda().view(B, pix, C)
    lib = _lib.lib()
    # a tile size that divides the pixel count and one that does not (1 = 1, 4097 = 17 * 241, 6145 = 5 * 1229)
    for tp in {1: (1, 4), 4097: (241, 256), 6145: (5, 256)}[pix]:
        def run(xw_):
            ratio = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
            out = torch.full_like(h, float("nan"))
            ts = _tile_sums(xw_, tp)
            check(lib.glare_mean_rescale_fused_bf16(ptr(h), ptr(xw_), int(x16), ptr(out), B, n, pix, ptr(hs), ptr(ts), tp, int(whole),
                                                    ptr(ratio), stream_handle()), "glare_mean_rescale_fused_bf16")
            assert torch.equal(_bits(out), _bits(ops.mean_rescale_fused(h, xw_, hs, ts, tp, whole_batch=whole)))
            return out, ratio.double()

        out, rk = run(xw)
        tag = "rescale_fused:%d:%d:%d:%d" % (n, whole, x16, tp)
        r64, rb = _check_rescale_output(out, h, xw, whole, per, tag + ":out")
        within(float(((rk - r64).abs() / rb).max()), 1.0, _tag(tag + ":ratio"))       # the ratio the kernel itself wrote
        if not whole:
            xw3 = xw.clone()
            xw3[1] = _r16(xw3[1].float() * 3) if x16 else xw3[1] * 3
            out3, _ = run(xw3)
            assert torch.equal(_bits(out3[0]), _bits(out[0])) and torch.equal(_bits(out3[2]), _bits(out[2]))


# ---- 3. layout conversions: bit-exact ---------------------------------------------------------------------------------------------
def test_layout_tiles_and_records_bit_exact(prec):
    g = torch.Generator().manual_seed(3)
    dt = ops.act_dtype()
    B = 2
    for C in (1, 3, 31, 33):
        for HW in (1, 31, 33, 1025):
            x = torch.randn(B, C, 1, HW, generator=g).cuda()
            want = x.permute(0, 2, 3, 1).contiguous()
            n32, n16 = ops.nchw_to_nhwc(x, bf16=False), ops.nchw_to_nhwc(x, bf16=True)
            assert n32.dtype == torch.float32 and n16.dtype == dt
            assert torch.equal(_bits(n32), _bits(want)) and torch.equal(_bits(n16), _bits(want.to(dt))), (C, HW)
            assert torch.equal(_bits(ops.nhwc_to_nchw(n32)), _bits(x)), (C, HW)
            assert torch.equal(_bits(ops.nhwc_to_nchw(n16)), _bits(want.to(dt).float().permute(0, 3, 1, 2).contiguous())), (C, HW)
    C, HW, pitch = 33, 33, 40
    x = torch.randn(B, C, 1, HW, generator=g).cuda()
    want = x.permute(0, 2, 3, 1).contiguous()
    for odt in (torch.float32, dt):
        for off in (0, 7):
            wide = torch.full((B, 1, HW, pitch), -7.0, dtype=odt, device="cuda")
            before = wide.clone()
            ops.nchw_to_nhwc(x, out=wide, out_off=off)
            assert torch.equal(_bits(wide[..., off:off + C]), _bits(want.to(odt))), (odt, off)
            assert torch.equal(wide[..., :off], before[..., :off]) and torch.equal(wide[..., off + C:], before[..., off + C:]), (odt, off)
        rec = torch.randn(B, 1, HW, pitch, generator=g).to(odt).cuda()
        got = ops.nhwc_to_nchw(rec, C=33, off=7)
        assert torch.equal(_bits(got), _bits(rec[..., 7:40].float().permute(0, 3, 1, 2).contiguous())), odt


# ---- 4. split_hilo: bit-exact -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (8, 8 * (4096 * 256 + 3)))
def test_split_hilo_bit_exact(prec, n):
    m, _ = _fmt()
    dt = ops.act_dtype()
    g = torch.Generator().manual_seed(4)
    # zeros, exactly representable values, exact ties (half way between two 16-bit values, towards an even and an odd neighbour)
    special = torch.tensor([0.0, -0.0, 1.0, -3.0, 1 + 2.0 ** -(m + 1), 1 + 3 * 2.0 ** -(m + 1), -(2 + 2.0 ** -m), 1.0e-3 * (1 + 2.0 ** -20)],
                           dtype=torch.float32)
    x = torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 6 - 4)
    x[:8] = special
    x[-8:] = special          # the large size: the vector only the loop's second trip reaches
    x = x.cuda()
    hi = ops.split_hilo(x)
    lo = hi._lo
    want_hi = x.to(dt)
    assert torch.equal(_bits(hi), _bits(want_hi))
    assert torch.equal(_bits(lo), _bits((x - want_hi.float()).to(dt)))
    # (`<=`: a remainder half way between two 16-bit values meets the bound exactly, and within() is strict)
    within(float(((x.double() - (hi.double() + lo.double())).abs() / (0.5 * ulp16(lo))).max()), 1.0 + 2.0 ** -40, _tag("split_hilo:%d" % n))


# ---- 5. GroupNorm -----------------------------------------------------------------------------------------------------------------
GN_EPS = 1e-6


def _gn_splits(HW):
    return max(1, min(64, HW // 128))


def _gn_exact(x, gamma, beta):
    """fp64 F.group_norm of the operands (x: [B, HW, C] on the device, any float type) -> [B, HW, C] fp64, before the activation"""
    y = F.group_norm(x.double().permute(0, 2, 1), 32, gamma.double(), beta.double(), eps=_f32(GN_EPS))
    return y.permute(0, 2, 1).contiguous()


def _swish64(y):
    return y * torch.sigmoid(y)


def _gn_fp32_coeffs(x, gamma, beta):
    """The statistics pass the header of gn.hip describes, in torch fp32 on the CPU: per (image, split) one-pass fp32 sums of x and
    x^2 -- per-thread chains over the split's pixels, then over the rows of the block, then over the group's channels --, the splits
    combined in fp64, var = E[x^2] - m^2, mean and rstd rounded to fp32.  Returns the per-(image, channel) fp32 pair of the apply pass,
    sc = rstd gamma and sh = beta - mean sc."""
    B, HW, C = x.shape
    cpg, ppi = C // 32, 256 // (C // 8)
    splits = _gn_splits(HW)
    per = -(-HW // splits)
    iters = -(-per // ppi)
    xp = F.pad(x, (0, 0, 0, splits * per - HW)).view(B, splits, per, C)              # zeros add exactly
    xp = F.pad(xp, (0, 0, 0, iters * ppi - per)).view(B, splits, iters, ppi, C)
    s = torch.zeros(B, splits, ppi, C)
    q = torch.zeros(B, splits, ppi, C)
    for i in range(iters):
        v = xp[:, :, i]
        s, q = s + v, q + v * v
    cs, cq = torch.zeros(B, splits, C), torch.zeros(B, splits, C)
    for r in range(ppi):
        cs, cq = cs + s[:, :, r], cq + q[:, :, r]
    cs, cq = cs.view(B, splits, 32, cpg), cq.view(B, splits, 32, cpg)
    gs, gq = torch.zeros(B, splits, 32), torch.zeros(B, splits, 32)
    for i in range(cpg):
        gs, gq = gs + cs[..., i], gq + cq[..., i]
    n = float(HW * cpg)
    mean = gs.double().sum(1) / n
    var = (gq.double().sum(1) / n - mean * mean).clamp_min(0.0)
    rstd = (1.0 / torch.sqrt(var + _f32(GN_EPS))).float()
    sc = rstd.repeat_interleave(cpg, 1) * gamma
    return sc, beta - mean.float().repeat_interleave(cpg, 1) * sc


def _gn_apply32(x, sc, sh):
    """max-error-wise the worse of the two fp32 forms of the apply pass (products rounded / contracted): [B, HW, C] each"""
    return x * sc[:, None] + sh[:, None], (x.double() * sc.double()[:, None] + sh.double()[:, None]).float()


def _gn_comparators(x, gamma, beta):
    """For the conditioning table only (CPU, x fp32 [B, HW, C]): the SAME fp32 apply pass fed by other statistics.
      exact   mean and variance in fp64, rounded to fp32 (what is left is the apply pass alone)
      2-pass  mean in fp32, then the centred second moment in fp32, both as contiguous reductions over the group (a strided
              torch reduction is off by several ulps of the mean and would be charged to the algorithm)"""
    B, HW, C = x.shape
    cpg = C // 32
    xg = x.view(B, HW, 32, cpg).permute(0, 2, 1, 3).reshape(B, 32, HW * cpg).contiguous()
    out = []
    for mean, var in ((xg.double().mean(2), xg.double().var(2, unbiased=False)),
                      (xg.mean(2), ((xg - xg.mean(2, keepdim=True)) ** 2).mean(2))):
        rstd = (1.0 / torch.sqrt(var.double() + _f32(GN_EPS))).float()
        sc = rstd.repeat_interleave(cpg, 1) * gamma
        out.append(_gn_apply32(x, sc, beta - mean.float().repeat_interleave(cpg, 1) * sc))
    return out


def _swish32(y):
    return y / (1.0 + torch.exp(-y))


def _gn_allowance(x_cpu32, gamma, beta, exact, swish):
    """S = 4 x the largest error against fp64 of the fp32 one-pass evaluation: the statistics allowance, measured on the reference
    side (4: the kernel's summation order is not torch's).  The apply pass y = x * sc + sh [-> swish] is evaluated in fp32 both with
    every product rounded and contracted to one rounding (a compiler may pick either); S takes the larger error.  (The elementwise
    apply runs as torch fp32 on the device: the same IEEE operations as on the CPU.)"""
    sc, sh = (t.cuda() for t in _gn_fp32_coeffs(x_cpu32, gamma.cpu(), beta.cpu()))
    x = x_cpu32.cuda()
    errs = []
    for y in _gn_apply32(x, sc, sh):
        y = _swish32(y) if swish else y
        errs.append(float((y.double() - exact).abs().max()))
    return 4.0 * max(errs), max(errs)


def _gn_params(C, g):
    return (torch.randn(C, generator=g) * 0.3 + 1).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()


def _gn_check_all_forms(x32, gamma, beta, tag, H=1, swishes=(False, True)):
    """x32: fp32 [B, HW, C] on the CPU.  plain: GroupNorm of round16(x); pair: of the hi / lo pair of x, output 16-bit or a pair."""
    B, HW, C = x32.shape
    hi = _r16(x32)
    lo = _r16(x32 - hi.float())
    x_pair = hi.float() + lo.float()                      # 22 bits: exact in fp32
    dhi, dlo = hi.cuda().view(B, H, HW // H, C), lo.cuda().view(B, H, HW // H, C)
    e_plain, e_pair = _gn_exact(hi.cuda(), gamma, beta), _gn_exact(x_pair.cuda(), gamma, beta)
    for swish in swishes:
        ex = _swish64(e_plain) if swish else e_plain
        S, emu = _gn_allowance(hi.float(), gamma, beta, ex, swish)
        within(emu, S, _tag("%s:plain:swish%d:S" % (tag, swish)))
        y = ops.groupnorm(dhi, gamma, beta, swish=swish)
        assert_rounded(y.view(B, HW, C), ex, S, "%s:plain:swish%d" % (tag, swish))
        ex = _swish64(e_pair) if swish else e_pair
        S, emu = _gn_allowance(x_pair, gamma, beta, ex, swish)
        within(emu, S, _tag("%s:pair:swish%d:S" % (tag, swish)))
        xin = dhi.clone()
        xin._lo = dlo
        y = ops.groupnorm(xin, gamma, beta, swish=swish, pair=False)
        assert getattr(y, "_lo", None) is None
        assert_rounded(y.view(B, HW, C), ex, S, "%s:pair_in:swish%d" % (tag, swish))
        y2 = ops.groupnorm(xin, gamma, beta, swish=swish, pair=True)
        assert torch.equal(_bits(y2), _bits(y))
        assert_pair(y2.view(B, HW, C), y2._lo.view(B, HW, C), ex, S, "%s:pair_out:swish%d" % (tag, swish))


# gn_splits = 1, 1, 1, 1, 1, 64; pixels per iteration 64 (C = 32) and 1 (C = 2048): every remainder of the x4 and x2 unrolled loops
@pytest.mark.parametrize("C", (32, 2048))
@pytest.mark.parametrize("HW", (1, 127, 128, 129, 255, 8193))
def test_groupnorm_split_and_unroll_edges(prec, HW, C):
    g = torch.Generator().manual_seed(HW + C)
    gamma, beta = _gn_params(C, g)
    x = torch.randn(2, HW, C, generator=g) * 2 + 0.5
    _gn_check_all_forms(x, gamma, beta, "gn:%dx%d" % (HW, C))


@pytest.mark.parametrize("HW", [k * 16 + d for k in (3, 5, 9) for d in (-1, 1)])
def test_groupnorm_remainders_c128(prec, HW):
    """C = 128: 16 pixels per iteration; 3, 5 and 9 iterations, one pixel short and one over"""
    g = torch.Generator().manual_seed(HW)
    gamma, beta = _gn_params(128, g)
    _gn_check_all_forms(torch.randn(2, HW, 128, generator=g) * 2 + 0.5, gamma, beta, "gn:%dx128" % HW)


def test_groupnorm_slice_of_a_wider_record(prec):
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 7, 41                                     # 287 pixels: two splits, 32 pixels per iteration, one short
    gamma, beta = _gn_params(64, g)
    rec = _r16(torch.randn(B, H, W, 128, generator=g) * 2 + 0.5)
    x = rec[..., 32:96].reshape(B, H * W, 64)
    for swish in (False, True):
        ex = _gn_exact(x.cuda(), gamma, beta)
        ex = _swish64(ex) if swish else ex
        S, _ = _gn_allowance(x.float(), gamma, beta, ex, swish)
        y = ops.groupnorm(rec.cuda(), gamma, beta, swish=swish, cin=64, in_off=32)
        assert y.shape == (B, H, W, 64)
        assert_rounded(y.view(B, H * W, 64), ex, S, "gn:slice:swish%d" % swish)


def test_groupnorm_images_do_not_mix(prec):
    """image 1 scaled by 100: the neighbours' partials are their own"""
    g = torch.Generator().manual_seed(6)
    B, HW, C = 3, 300, 128                                 # two splits
    gamma, beta = _gn_params(C, g)
    x = torch.randn(B, 1, HW, C, generator=g) * 2 + 0.5
    x2 = x.clone()
    x2[1] *= 100
    hi, hi2 = _r16(x).cuda(), _r16(x2).cuda()
    y, y2 = ops.groupnorm(hi, gamma, beta), ops.groupnorm(hi2, gamma, beta)
    assert torch.equal(_bits(y[0]), _bits(y2[0])) and torch.equal(_bits(y[2]), _bits(y2[2]))
    hi._lo, hi2._lo = _r16(x - _r16(x).float()).cuda(), _r16(x2 - _r16(x2).float()).cuda()
    for pair in (False, True):
        y, y2 = ops.groupnorm(hi, gamma, beta, pair=pair), ops.groupnorm(hi2, gamma, beta, pair=pair)
        assert torch.equal(_bits(y[0]), _bits(y2[0])) and torch.equal(_bits(y[2]), _bits(y2[2]))
        if pair:
            assert torch.equal(_bits(y._lo[0]), _bits(y2._lo[0])) and torch.equal(_bits(y._lo[2]), _bits(y2._lo[2]))


GN_COND_HEADER = """GroupNorm against the conditioning of a group (ratio = mean / std of the group's values), measured on an MI355X.
Written by tests/test_gpu_streaming_edges.py::test_groupnorm_conditioning (B 2, HW 1025, C 128, gamma ~ N(1, 0.3), no activation);
every figure is the largest |value - fp64 F.group_norm| over the tensor.
  form    plain = GroupNorm of a 16-bit tensor, 16-bit output (kernel: includes that output's rounding, 0.5 ulp16);
          pair = of a hi / lo pair, output a hi / lo pair, read back as hi + lo
  kernel  the HIP kernels
  S       the test's statistics allowance = 4 x 1-pass
  1-pass  the algorithm of gn.hip in torch fp32: one-pass fp32 sums, fp64 combine, E[x^2] - m^2, fp32 apply
  2-pass  the same fp32 apply on two-pass fp32 statistics (mean, then the centred second moment)
  exact   the same fp32 apply on fp64 statistics rounded to fp32: the apply pass alone
  used    the largest |error| / (rounding + S) of any element: the share of the per-element bound in use

prec  form    ratio        kernel             S        1-pass        2-pass         exact      used
"""
_gn_cond_rows = {}


@pytest.mark.parametrize("ratio", (0.25, 8.0, 32.0))
def test_groupnorm_conditioning(prec, ratio):
    """group mean / group std = ratio: the one-pass E[x^2] - m^2 loses ~ratio^2 ulps of the variance; S grows with it, the bound's
    form does not change.  The table of this session's rows, with its header, is rewritten as gn_conditioning.txt under $GLARE_OUT_DIR
    (default out/), where the tools' results go; profiles/gn_conditioning.txt is a copy of it."""
    g = torch.Generator().manual_seed(int(ratio * 4))
    B, HW, C = 2, 1025, 128
    gamma, beta = _gn_params(C, g)
    x32 = torch.randn(B, HW, C, generator=g) + ratio
    hi = _r16(x32)
    lo = _r16(x32 - hi.float())
    for form, xc in (("plain", hi.float()), ("pair", hi.float() + lo.float())):
        ex = _gn_exact(xc.cuda(), gamma, beta)
        S, emu = _gn_allowance(xc, gamma, beta, ex, False)
        exact_stats, two = (max(float((y.cuda().double() - ex).abs().max()) for y in ys)
                            for ys in _gn_comparators(xc, gamma.cpu(), beta.cpu()))
        xin = hi.cuda().view(B, 1, HW, C)
        if form == "pair":
            xin._lo = lo.cuda().view(B, 1, HW, C)
            y = ops.groupnorm(xin, gamma, beta, swish=False, pair=True)
            got = y.double() + y._lo.double()
            used = assert_pair(y.view(B, HW, C), y._lo.view(B, HW, C), ex, S, "gn_cond:%g:pair" % ratio)
        else:
            y = ops.groupnorm(xin, gamma, beta, swish=False)
            got = y.double()
            used = assert_rounded(y.view(B, HW, C), ex, S, "gn_cond:%g:plain" % ratio)
        kerr = float((got.view(B, HW, C) - ex).abs().max())
        within(emu, S, _tag("gn_cond:%g:%s:S" % (ratio, form)))
        _gn_cond_rows[(prec, ratio, form)] = ("%-5s %-6s %6g  %12.4e  %12.4e  %12.4e  %12.4e  %12.4e  %8.4f\n"
                                              % (prec, form, ratio, kerr, S, emu, two, exact_stats, used))
    out = os.path.join(ROOT, os.environ.get("GLARE_OUT_DIR", "out"))
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "gn_conditioning.txt"), "w") as f:
            f.write(GN_COND_HEADER + "".join(_gn_cond_rows[k] for k in sorted(_gn_cond_rows)))
    except OSError as e:       # a read-only tree: the checks above have run, only the table is lost -- say so
        warnings.warn("gn_conditioning.txt not written: %s" % e)


# ---- 6. flow per-pixel kernels (fp32 state) ---------------------------------------------------------------------------------------
FLOW_EPS = 1e-4


def _scale64(x):
    """s = sigmoid(x + 2) + eps in fp64 and the relative error bound of its fp32 evaluation 1 / (1 + expf(-(x + 2))) + eps:
    a = x + 2 rounds once, which moves e = expf(-a) by |a| U relative; expf itself 2 ulp = 4 U; 1 + e rounds once and damps e's error
    by e / (1 + e) = 1 - sigmoid; the division is correctly rounded (1 U); + eps rounds once:  ((1 - sig) (4 + |a|) + 3) U"""
    a = x.double() + 2.0
    return torch.sigmoid(a) + _f32(FLOW_EPS), (torch.sigmoid(-a) * (4.0 + a.abs()) + 3.0) * U


def _affine64(v, ev, M, t):
    """M v + t as three chained fmas per row: the input errors through |M|, 3 roundings on the magnitudes of the terms"""
    M64, t64 = M.double().to(v.device), t.double().to(v.device)
    out = v @ M64.t() + t64
    mag = v.abs() @ M64.abs().t() + t64.abs()
    return out, ev @ M64.abs().t() + 3 * U * mag


def _unscale64(z, ez, x_scale, shift):
    """z / s - shift: the division (1 U) on top of s's own error, the subtraction (1 U)"""
    s, rs = _scale64(x_scale)
    q = z / s
    sh = shift.double()
    return q - sh, ez / s + q.abs() * (rs + U) + U * (q.abs() + sh.abs())


def _flow_h1_case(B, H, W, pitch, off, g):
    z = torch.randn(B, H, W, 3, generator=g)
    z[..., 0] += 10.0 * (torch.arange(B).view(B, 1, 1) + 1)       # a tap that leaks across an image border or a row wrap is an O(10) error
    ftA = torch.randn(B, H, W, pitch, generator=g)
    wz = torch.randn(64, 9, generator=g) * 0.1
    z0 = z[..., 0].double().unsqueeze(1)
    w64 = wz.double().view(64, 1, 3, 3)
    a64 = ftA[..., off:off + 64].double()
    exact = (F.conv2d(z0, w64, None, 1, 1).permute(0, 2, 3, 1) + a64).cuda()
    mag = (F.conv2d(z0.abs(), w64.abs(), None, 1, 1).permute(0, 2, 3, 1) + a64.abs()).cuda()
    return z.cuda(), ftA.cuda(), wz.cuda(), exact, 10 * U * mag      # 9 chained fmas on the accumulator (9 roundings) + 1 spare


@pytest.mark.parametrize("pitch,off", ((192, 64), (68, 4)))
@pytest.mark.parametrize("H,W", ((1, 1), (1, 7), (7, 1), (3, 5)))
def test_flow_h1_per_element(prec, H, W, pitch, off):
    g = torch.Generator().manual_seed(H * 8 + W + pitch)
    z, ftA, wz, exact, tol = _flow_h1_case(3, H, W, pitch, off, g)
    tag = "flow_h1:%dx%d:%d" % (H, W, pitch)
    assert_f32(train_ops.flow_h1_raw(z, ftA, off, wz), exact, tol, tag + ":raw")
    relu = exact.clamp_min(0.0)
    assert_rounded(ops.flow_h1(z, ftA, off, wz), relu, tol, tag)
    out = torch.empty(3, H, W, 64, dtype=ops.act_dtype(), device="cuda")
    out._lo = torch.empty_like(out)
    got = ops.flow_h1(z, ftA, off, wz, out=out)
    assert torch.equal(_bits(got), _bits(ops.flow_h1(z, ftA, off, wz)))
    assert_pair(got, got._lo, relu, tol, tag + ":pair")


def _flow_mt(g):
    return torch.randn(3, 3, generator=g), torch.randn(3, generator=g)


@pytest.mark.parametrize("pitch,off", ((16, 8), (8, 0)))
@pytest.mark.parametrize("npix", (1, 257, 4096 * 256 + 5))
def test_flow_tail_and_affine3_per_element(prec, npix, pitch, off):
    g = torch.Generator().manual_seed(npix % 1000 + pitch)
    z = torch.randn(1, 1, npix, 3, generator=g).cuda()
    h4 = torch.randn(1, 1, npix, 4, generator=g).cuda()
    hF = torch.randn(1, 1, npix, pitch, generator=g).cuda()
    M, t = _flow_mt(g)
    z64, f = z.double(), hF[..., off:off + 6]
    zero = torch.zeros_like(z64[..., 0])
    v1, e1 = _unscale64(z64[..., 1], zero, h4[..., 1], h4[..., 0])
    v2, e2 = _unscale64(z64[..., 2], zero, h4[..., 3], h4[..., 2])
    v = [_unscale64(z64[..., 0], zero, f[..., 1], f[..., 0]), _unscale64(v1, e1, f[..., 3], f[..., 2]), _unscale64(v2, e2, f[..., 5], f[..., 4])]
    exact, tol = _affine64(torch.stack([a for a, _ in v], -1), torch.stack([e for _, e in v], -1), M, t)
    got = z.clone()
    ops.flow_tail(got, h4, hF, off, M.flatten().tolist(), t.tolist(), eps=FLOW_EPS)
    assert_f32(got, exact, tol, "flow_tail:%d:%d" % (npix, pitch))
    exact, tol = _affine64(z64, torch.zeros_like(z64), M, t)
    got = z.clone()
    train_ops.flow_affine3_(got, M.flatten().tolist(), t.tolist())
    assert_f32(got, exact, tol, "flow_affine3:%d" % npix)


def _block_partials(L, el, mag, bps, terms_per_pixel):
    """[B, P] per-pixel log-determinant terms -> [B, bps]: block blk of an image owns the pixels q with (q // 256) % bps == blk.
    Tolerance: the terms' own errors + the fp32 chain (terms_per_pixel per trip of the per-block loop, 6 shuffles, 3 adds)"""
    B, P = L.shape
    idx = ((torch.arange(P, device=L.device) // 256) % bps)
    z = torch.zeros(B, bps, dtype=torch.float64, device=L.device)
    adds = terms_per_pixel * -(-P // (bps * 256)) + 9
    return z.index_add(1, idx, L), z.index_add(1, idx, el) + adds * U * z.index_add(1, idx, mag)


@pytest.mark.parametrize("P,want_bps", ((1, 1), (255, 1), (257, 2), (16385, 64)))
def test_flow_fwd_pre_and_post_per_element_and_per_block(prec, P, want_bps):
    g = torch.Generator().manual_seed(P)
    B = 3
    bps = ops.flow_blocks_per_sample(P)
    assert bps == want_bps
    z = torch.randn(B, 1, P, 3, generator=g).cuda()
    hF = (torch.randn(B, 1, P, 16, generator=g) + 0.5 * torch.arange(B).view(B, 1, 1, 1)).cuda()     # a swapped sample index shows
    h4 = (torch.randn(B, 1, P, 4, generator=g) + 0.5 * torch.arange(B).view(B, 1, 1, 1)).cuda()
    M, t = _flow_mt(g)
    # pre: z' = M z + t; out = (z' + shift) * s; partial = sum of log s0 + log s1 + log s2
    f = hF[..., 8:14].double()
    zz, ez = _affine64(z.double(), torch.zeros_like(z.double()), M, t)
    sc = [_scale64(f[..., 2 * i + 1]) for i in range(3)]
    s, rs = torch.stack([a for a, _ in sc], -1), torch.stack([b for _, b in sc], -1)
    w = zz + f[..., 0::2]
    exact = w * s
    tol = (ez + U * (zz.abs() + f[..., 0::2].abs())) * s + exact.abs() * (rs + U)      # the sum rounds once, the product once
    logs = torch.log(s)
    el = rs + 4 * U * logs.abs()                                                         # logf: s's error / s, and 2 ulp of its own
    pex, ptol = _block_partials(logs.sum(-1).view(B, P), el.sum(-1).view(B, P), logs.abs().sum(-1).view(B, P), bps, 3)
    Mt = torch.cat([M.flatten(), t]).cuda()
    for form in ("host", "dev", "dev_out"):
        part = torch.full((B * bps,), float("nan"), dtype=torch.float32, device="cuda")
        got = z.clone()
        if form == "host":
            ops.flow_fwd_pre(got, hF, 8, M.flatten().tolist(), t.tolist(), FLOW_EPS, part)
        elif form == "dev":
            ops.flow_fwd_pre(got, hF, 8, None, None, FLOW_EPS, part, Mt_dev=Mt)
        else:
            src = z.clone()
            got = torch.full_like(z, float("nan"))
            ops.flow_fwd_pre(src, hF, 8, None, None, FLOW_EPS, part, Mt_dev=Mt, out=got)
            assert torch.equal(_bits(src), _bits(z))
        assert_f32(got, exact, tol, "flow_fwd_pre:%d:%s" % (P, form))
        assert_f32(part.view(B, bps), pex, ptol, "flow_fwd_pre:%d:%s:partial" % (P, form))
    # post: z[1:] = (z[1:] + shift) * s; channel 0 passes through
    h64, z64 = h4.double(), z.double()
    sc = [_scale64(h64[..., 1]), _scale64(h64[..., 3])]
    s, rs = torch.stack([a for a, _ in sc], -1), torch.stack([b for _, b in sc], -1)
    exact = (z64[..., 1:] + h64[..., 0::2]) * s
    tol = U * (z64[..., 1:].abs() + h64[..., 0::2].abs()) * s + exact.abs() * (rs + U)
    logs = torch.log(s)
    el = rs + 4 * U * logs.abs()
    pex, ptol = _block_partials(logs.sum(-1).view(B, P), el.sum(-1).view(B, P), logs.abs().sum(-1).view(B, P), bps, 2)
    for form in ("in_place", "out"):
        part = torch.full((B * bps,), float("nan"), dtype=torch.float32, device="cuda")
        if form == "in_place":
            got = z.clone()
            ops.flow_fwd_post(got, h4, FLOW_EPS, part)
        else:
            src = z.clone()
            got = torch.full_like(z, float("nan"))
            ops.flow_fwd_post(src, h4, FLOW_EPS, part, out=got)
            assert torch.equal(_bits(src), _bits(z))
        assert torch.equal(_bits(got[..., 0]), _bits(z[..., 0]))
        assert_f32(got[..., 1:].contiguous(), exact, tol, "flow_fwd_post:%d:%s" % (P, form))
        assert_f32(part.view(B, bps), pex, ptol, "flow_fwd_post:%d:%s:partial" % (P, form))


@pytest.mark.parametrize("n_rows", (0, 1, 4))
@pytest.mark.parametrize("P", (1, 257, 16385))
def test_flow_nll_reduce_per_image(prec, P, n_rows):
    g = torch.Generator().manual_seed(P + n_rows)
    B = 3
    bps = ops.flow_blocks_per_sample(P)
    z = torch.randn(B, 1, P, 3, generator=g).cuda()
    other = torch.randn(B, 1, P, 3, generator=g).cuda()
    R = max(n_rows, 1)
    partial = (torch.randn(R, B * bps, generator=g) + 0.37 * torch.arange(R * B * bps).view(R, B * bps)).cuda()   # distinct per (row, image, block)
    p64 = partial[:n_rows].double().view(n_rows, B, bps)
    log2pi = _f32(1.8378770664093453)
    for name, mean in (("self", z), ("other", other)):
        out = ops.flow_nll_reduce(z, mean, partial, n_rows)
        assert out.dtype == torch.float64 and out.shape == (B, 2)
        tag = "flow_nll:%d:%d:%s" % (P, n_rows, name)
        if n_rows == 0:
            assert torch.equal(out[:, 0], torch.zeros(B, dtype=torch.float64, device="cuda"))
        else:    # fp32 values accumulated in fp64: its rounding only
            within(float(((out[:, 0] - p64.sum((0, 2))).abs() / (n_rows * bps * 2.0 ** -52 * p64.abs().sum((0, 2)))).max()), 1.0, _tag(tag + ":ld"))
        d = (z.double() - mean.double()).view(B, -1)
        terms = -0.5 * (d * d + log2pi)
        # d rounds once (2 U on d^2), d * d once: 3 U d^2, halved; then the fp64 accumulation of 3 P terms
        tol = 1.5 * U * (d * d).sum(1) + 3 * P * 2.0 ** -52 * terms.abs().sum(1)
        within(float(((out[:, 1] - terms.sum(1)).abs() / tol).max()), 1.0, _tag(tag + ":lp"))
