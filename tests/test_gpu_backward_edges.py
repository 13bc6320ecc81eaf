"""GPU: the ADJOINTS of the streaming kernels test_gpu_streaming_edges.py pins (csrc/flow_bwd.hip; GroupNorm, mix, mean rescale and
act backward of csrc/train_ops.hip) PER ELEMENT against the fp64 restatements of tests/backward_fp64.py (themselves checked against
fp64 autograd on the CPU: test_backward_fp64_host.py), at the shapes where their index arithmetic changes regime: a sample boundary
inside a block, the second trip of a grid-stride loop, an empty or ragged split, every unroll remainder, a slice of a wider record,
blocks that own no pixel.  No element is left out of any comparison.

The bounds follow the streaming file's rule (fp64_bounds.py):
    16-bit outputs   |got - exact| <= 0.5 ulp16(exact) + slack
    fp32 outputs     |got - exact| <= slack
`slack` is counted from the kernel's own expression and stated next to each call: for an elementwise expression (number of fp32
roundings) U times the magnitudes of the terms (never their cancelled sum), for a sum (additions behind that partial) U sum|terms|,
plus the propagated error of whatever the expression reads.  An fma counts as the one rounding of its chain; a compiler that
contracts a product into a sum only removes roundings.  Operands are rounded to the 16-bit format before either side sees them
(the fp32 flow state stays fp32).  Every check goes through tolerances.within(measured / bound, 1.0)."""
import math

import pytest
import torch

import backward_fp64 as R
from fp64_bounds import U, _bits, _f32, _fmt, _r16, _tag, assert_rounded
from glare_amd import _lib, ops, train_ops
from glare_amd._lib import check, host_f32, ptr, stream_handle
from test_gpu_streaming_edges import FLOW_EPS, GN_EPS, _scale64
from tolerances import within

pytestmark = pytest.mark.gpu

G_SAMPLE = (0.7, 0.0, -1.3)          # the per-sample upstream gradient of logp / logdet: distinct, a zero, a negative value


@pytest.fixture(params=("bf16", "fp16"))
def prec(request):
    with ops.use_precision(request.param):
        yield request.param


# ---- shared helpers ---------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    """err / bound per element; 0 where the error is 0 (a gradient that is exactly zero, met exactly, has bound 0 as well)"""
    return torch.where(err == 0, torch.zeros_like(err), err / bound)


def check_f32(got32, exact64, tol64, tag):
    """an fp32 result, every element: |got - exact| <= tol"""
    assert got32.dtype == torch.float32 and got32.shape == exact64.shape, (got32.dtype, got32.shape, exact64.shape)
    return within(float(_ratio((got32.double() - exact64).abs(), tol64).max()), 1.0, _tag(tag))


def _sigmoid_rel(a, arg_roundings):
    """sigmoid(a) in fp64 and the relative error bound of its fp32 evaluation 1 / (1 + exp(-a)): the count of the streaming file's
    _scale64 without the roundings of `a + 2` and `+ eps`.  e = exp(-a): expf 2 ulp = 4 U, and |a| U for each rounding on the way to
    the exponent (arg_roundings; __expf is exp2 of a * log2(e): the product and the rounded constant, 2, which expf's range
    reduction does not have); 1 + e rounds once and damps e's error by 1 - sigmoid; the division 1 U."""
    return torch.sigmoid(a), (torch.sigmoid(-a) * (4.0 + arg_roundings * a.abs()) + 2.0) * U


def _reduce_depth(parts, n):
    """additions behind one element of glare_reduce_parts_f32: one chain, or (many parts of few elements) 16 interleaved chains
    and the 15 additions that join them"""
    return -(-parts // 16) + 15 if parts >= 32 and n <= 65536 else parts


def _block_sum(values, block_of, n_blocks):
    """[n, k] fp64 -> [n_blocks, k]: the sum over the rows each block owns"""
    return torch.zeros(n_blocks, values.shape[1], dtype=torch.float64, device=values.device).index_add(0, block_of, values)


def _sample_grad(B):
    return torch.tensor(G_SAMPLE[:B] if B > 1 else (G_SAMPLE[0],), dtype=torch.float32, device="cuda")


def _coupling_bounds(g, pre_mag, e_pre, shift, raw, gl):
    """The two gradients of one coupling channel as the kernels evaluate them (flow_post_bwd_kernel, flow_pre_bwd_kernel):
        sg = sigmoid(raw + 2), s = sg + eps                    relative error rs each (_scale64: the count includes + eps)
        gp = g * s                                             rs + the product: |gp| (rs + U)
        gs = g * (pre + shift) + gl / s                        pre + shift rounds once (on |pre| + |shift|), the product once, the sum
                                                               once on both terms; gl / s: rs + the division
        gr = gs * sg * (1 - sg)                                1 - sg carries sg's ABSOLUTE error (as _mix_exact does) + its own
                                                               rounding; two products
    pre_mag, e_pre: magnitude of the terms of `pre` and its own error (0 for a stored value).  -> (e_gp, e_gr)"""
    s, rs = _scale64(raw)
    sg = torch.sigmoid(raw + 2.0)
    e_gp = (g * s).abs() * (rs + U)
    w_mag = pre_mag + shift.abs()
    q = (gl / s).abs()
    mag_gs = g.abs() * w_mag + q
    e_gs = g.abs() * (e_pre + 3 * U * w_mag) + q * (rs + 2 * U)
    e_sg = rs * sg
    e_1m = e_sg + U * (1.0 - sg)
    e_gr = e_gs * sg * (1.0 - sg) + mag_gs * (e_sg * (1.0 - sg) + sg * e_1m + 2 * U * sg * (1.0 - sg))
    return e_gp, e_gr


# ---- 1. flow_nll_backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pps", (1, 85, 342))
def test_flow_nll_backward_per_element(prec, pps):
    """3, 255 and 1026 elements per sample: no multiple of 256, a sample boundary inside a block"""
    g = torch.Generator().manual_seed(pps)
    B = 3
    z, mean = (torch.randn(B, 1, pps, 3, generator=g).cuda() for _ in range(2))
    glp = _sample_grad(B)
    gz, gmean = train_ops.flow_nll_backward(z, mean, glp)
    egz, egm = R.nll_backward(z.double(), mean.double(), glp.double())
    tol = 2 * U * (1 + U) * egm.abs()          # g = gl * (z - mean): the difference rounds once, the product once
    check_f32(gmean, egm, tol, "nll_bwd:%d:gmean" % pps)
    check_f32(gz, egz, tol, "nll_bwd:%d:gz" % pps)
    assert torch.equal(_bits(gz), _bits(gmean) ^ torch.tensor(-2 ** 31, dtype=torch.int32, device="cuda"))     # gz = -gmean, bit for bit


# ---- 2. flow_post_backward_ -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,pps", ((1, 1), (1, 255), (1, 257), (3, 171)))
def test_flow_post_backward_per_element(prec, B, pps):
    g = torch.Generator().manual_seed(B * 1000 + pps)
    gz0, z_pre = (torch.randn(B, 1, pps, 3, generator=g).cuda() for _ in range(2))
    h4 = torch.randn(B, 1, pps, 4, generator=g)
    h4[..., 1::2] = torch.rand(B, 1, pps, 2, generator=g) * 20 - 12          # raw over [-12, 8]: the sigmoid saturates on both sides
    h4 = h4.cuda()
    eps = _f32(FLOW_EPS)                                                     # what FlowUpsamplerNet passes (affine_eps)
    for gl in ([torch.tensor([v], dtype=torch.float32, device="cuda") for v in (0.0, -0.9)] if B == 1 else [_sample_grad(B)]):
        gz = gz0.clone()
        gh4 = torch.full((B, 1, pps, 8), float("nan"), dtype=ops.act_dtype(), device="cuda")
        assert train_ops.flow_post_backward_(gz, z_pre, h4, gl, FLOW_EPS, out=gh4) is gh4
        egz, egh = R.post_backward(gz0.double(), z_pre.double(), h4.double(), gl.double(), eps)
        tag = "post_bwd:%dx%d:%g" % (B, pps, float(gl[0]))
        gl64, zero = R.per_sample(gl.double(), gz0[..., 0]), torch.zeros_like(egz[..., 0])
        bounds = [_coupling_bounds(gz0[..., 1 + c].double(), z_pre[..., 1 + c].double().abs(), zero, h4[..., 2 * c].double(),
                                   h4[..., 2 * c + 1].double(), gl64) for c in range(2)]
        assert torch.equal(_bits(gz[..., 0]), _bits(gz0[..., 0]))
        check_f32(gz[..., 1:].contiguous(), egz[..., 1:], torch.stack([b[0] for b in bounds], -1), tag + ":gz")
        assert_rounded(gh4[..., :4].contiguous(), egh, torch.stack([bounds[0][0], bounds[0][1], bounds[1][0], bounds[1][1]], -1),
                       tag + ":gh4")
        assert int(_bits(gh4[..., 4:]).abs().max()) == 0          # lanes 4..7 of every record: zero bits


# ---- 3. flow_h1_backward_ ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch,off", ((64, 0), (192, 64), (72, 8)))
@pytest.mark.parametrize("B,H,W", ((1, 1, 1), (1, 1, 9), (1, 7, 1), (2, 3, 5), (2, 5, 37), (1, 91, 91)))
def test_flow_h1_backward_per_element_and_per_block(prec, B, H, W, pitch, off):
    """(2, 3, 5) and (2, 5, 37): two images of very different scale (x64 on g, x8 + 20 on z0), so that a tap which leaks across the
    batch boundary or a row wrap is far over the bound; (2, 5, 37): blocks of 32 pixels straddle the rows of 37;
    (1, 91, 91) = 8281 pixels = 66 248 threads > 256 x 256: blocks 0..2 take a second trip."""
    g = torch.Generator().manual_seed(H * 100 + W + pitch)
    grec = torch.randn(B, H, W, pitch, generator=g)
    z_pre = torch.randn(B, H, W, 3, generator=g)
    if B > 1:
        grec[1] *= 64
        z_pre[1] = z_pre[1] * 8 + 20
    grec, z_pre = _r16(grec).cuda(), z_pre.cuda()
    wz = (torch.randn(64, 9, generator=g) * 0.1).cuda()
    gz0 = torch.randn(B, H, W, 3, generator=g).cuda()
    lib = _lib.lib()
    npix = B * H * W
    nb = int(lib.glare_flow_bwd_blocks(npix))
    assert nb == min(256, -(-npix * 8 // 256))
    trips = -(-npix * 8 // (nb * 256))
    assert trips == (2 if npix == 8281 else 1)

    def run():
        gz = gz0.clone()
        part = torch.full((nb, 576), float("nan"), dtype=torch.float32, device="cuda")
        check(lib.glare_flow_h1_backward_f32(ptr(gz), ptr(grec), pitch, off, ptr(z_pre), ptr(wz), B, H, W, ptr(part), stream_handle()),
              "glare_flow_h1_backward_f32")
        return gz, part

    gz, part = run()
    gz2, part2 = run()
    assert torch.equal(_bits(gz), _bits(gz2)) and torch.equal(_bits(part), _bits(part2))          # the same bits, run to run
    gzw = gz0.clone()
    dw = train_ops.flow_h1_backward_(gzw, grec, off, z_pre, wz)
    assert torch.equal(_bits(gzw), _bits(gz)) and dw.shape == (64, 9)
    tag = "h1_bwd:%dx%dx%d:%d" % (B, H, W, pitch)
    g64, z0, w64 = grec[..., off:off + 64].double(), z_pre[..., 0].double(), wz.double()
    # gz[..., 0] += dz: dz = 72 chained fmas (9 taps x 8 channels of the thread) and 3 shuffle additions over the 8 threads of a pixel,
    # on sum |g| |w|; then the += rounds once on |gz| + |dz|
    mag = R.h1_backward_data(g64.abs(), w64.abs())
    check_f32(gz[..., 0].contiguous(), gz0[..., 0].double() + R.h1_backward_data(g64, w64), 76 * U * mag + U * gz0[..., 0].double().abs(),
              tag + ":gz0")
    assert torch.equal(_bits(gz[..., 1:]), _bits(gz0[..., 1:]))
    # block blk owns the pixels (blk * 256 + k * nb * 256 + t) >> 3, t < 256, k = 0, 1, ...: 32 pixels per trip.  One fma per trip and
    # thread, 3 shuffle additions over the 8 pixels of a wave with the same channel group, 2 over the four waves
    terms = R.h1_filter_terms(g64, z0).view(npix, 576)
    block_of = ((8 * torch.arange(npix, device="cuda")) // 256) % nb
    pex, pmag = _block_sum(terms, block_of, nb), _block_sum(terms.abs(), block_of, nb)
    worst = _ratio((part.double() - pex).abs(), (trips + 5) * U * pmag).amax(1)
    bad = torch.nonzero(worst >= 1).flatten().tolist()
    assert not bad, "%s: partials of blocks %s off by %s x the bound" % (tag, bad, [float(worst[b]) for b in bad])
    within(float(worst.max()), 1.0, _tag(tag + ":partials"))
    check_f32(dw, terms.sum(0).view(64, 9), ((trips + 5 + _reduce_depth(nb, 576)) * U * terms.abs().sum(0)).view(64, 9), tag + ":dw")


# ---- 4. flow_pre_backward_ --------------------------------------------------------------------------------------------------------
PRE_M = ((0.9, -0.7, 0.3), (0.4, 1.1, -0.6), (-0.8, 0.5, 0.7))          # clearly not symmetric: M^T gy is not M gy
PRE_T = (0.3, -0.2, 0.5)


@pytest.mark.parametrize("f_pitch,f_off", ((8, 0), (24, 8), (12, 4)))
@pytest.mark.parametrize("B,pps", ((1, 1), (1, 300), (3, 171), (1, 65537)))
def test_flow_pre_backward_per_element_and_per_block(prec, B, pps, f_pitch, f_off):
    """One pixel per thread on a grid sized for 8 threads per pixel (glare_flow_bwd_blocks): 300 pixels fill 2 of 10 blocks, 65537
    pixels give pixel 65536 to block 0's second trip."""
    g = torch.Generator().manual_seed(B * 1000 + pps % 1000 + f_pitch)
    M32, t32 = torch.tensor(PRE_M, dtype=torch.float32), torch.tensor(PRE_T, dtype=torch.float32)
    assert float((M32 - M32.t()).abs().max()) > 0.5 and float(t32.abs().min()) > 0
    Mt_dev = torch.cat([M32.flatten(), t32]).cuda()
    M64, t64 = M32.double().cuda(), t32.double().cuda()
    gz0, z_in = (torch.randn(B, 1, pps, 3, generator=g).cuda() for _ in range(2))
    hF = torch.randn(B, 1, pps, f_pitch, generator=g)
    hF[..., f_off + 1:f_off + 6:2] *= 3
    hF = hF.cuda()
    gl = _sample_grad(B)
    eps = _f32(FLOW_EPS)
    lib = _lib.lib()
    npix = B * pps
    nb = int(lib.glare_flow_bwd_blocks(npix))
    assert nb == min(256, -(-npix * 8 // 256))
    trips = -(-npix // (nb * 256))
    assert trips == (2 if npix == 65537 else 1)
    Ma, ta = host_f32(M32.flatten().tolist(), 9), host_f32(t32.tolist(), 3)
    # the reference and the bounds
    f6 = hF[..., f_off:f_off + 6].double()
    egz, egf, gy = R.pre_backward(gz0.double(), z_in.double(), f6, gl.double(), M64, t64, eps)
    az = z_in.double().abs()
    ymag = az @ M64.abs().t() + t64.abs()                                    # y = M z + t: three chained fmas, 3 roundings on its terms
    gl64 = R.per_sample(gl.double(), gz0[..., 0])
    bounds = [_coupling_bounds(gz0[..., i].double(), ymag[..., i], 3 * U * ymag[..., i], f6[..., 2 * i], f6[..., 2 * i + 1], gl64)
              for i in range(3)]
    e_gy = torch.stack([b[0] for b in bounds], -1)
    e_gf = torch.stack([b[k] for b in bounds for k in (0, 1)], -1)
    # gz = M^T gy: each term through its product and the two additions, on top of gy's own error
    tol_gz = e_gy @ M64.abs() + 3 * U * (gy.abs() @ M64.abs())
    # partial[blk][12]: block blk owns the pixels blk * 256 + t + k * nb * 256.  One fma (or addition) per trip and thread, 6 shuffle
    # additions, 2 over the four waves; the terms carry gy's error
    terms = R.pre_terms(gy, z_in.double()).view(npix, 12)
    e_terms = R.pre_terms(e_gy, az).view(npix, 12)
    block_of = (torch.arange(npix, device="cuda") // 256) % nb
    pex = _block_sum(terms, block_of, nb)
    ptol = _block_sum(e_terms, block_of, nb) + (trips + 8) * U * _block_sum(terms.abs(), block_of, nb)
    filled = min(nb, -(-npix // 256))                                         # blocks that own a pixel
    assert filled <= nb and float(ptol[filled:].abs().max() if filled < nb else 0.0) == 0.0
    for gf_pitch, gf_off in ((8, 0), (24, 8)):
        res = {}
        for form in ("host", "dev"):
            gz = gz0.clone()
            ghF = torch.full((B, 1, pps, gf_pitch), -7.0, dtype=ops.act_dtype(), device="cuda")
            part = torch.full((nb, 12), float("nan"), dtype=torch.float32, device="cuda")
            if form == "host":
                check(lib.glare_flow_fwd_pre_backward_f32(ptr(gz), ptr(z_in), ptr(hF), f_pitch, f_off, ptr(gl), B, pps, Ma, ta, FLOW_EPS,
                                                          ptr(ghF), gf_pitch, gf_off, ptr(part), stream_handle()),
                      "glare_flow_fwd_pre_backward_f32")
            else:
                check(lib.glare_flow_fwd_pre_backward_dev_f32(ptr(gz), ptr(z_in), ptr(hF), f_pitch, f_off, ptr(gl), B, pps, ptr(Mt_dev),
                                                              FLOW_EPS, ptr(ghF), gf_pitch, gf_off, ptr(part), stream_handle()),
                      "glare_flow_fwd_pre_backward_dev_f32")
            res[form] = (gz, ghF, part)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(res["host"], res["dev"]))          # the two forms: the same bits
        gz, ghF, part = res["dev"]
        tag = "pre_bwd:%dx%d:%d:%d" % (B, pps, f_pitch, gf_pitch)
        check_f32(gz, egz, tol_gz, tag + ":gz")
        assert_rounded(ghF[..., gf_off:gf_off + 6].contiguous(), egf, e_gf, tag + ":ghF")
        assert int(_bits(ghF[..., gf_off + 6:gf_off + 8]).abs().max()) == 0          # lanes 6 and 7 of the written record
        sentinel = torch.full_like(ghF, -7.0)
        assert torch.equal(_bits(ghF[..., :gf_off]), _bits(sentinel[..., :gf_off]))
        assert torch.equal(_bits(ghF[..., gf_off + 8:]), _bits(sentinel[..., gf_off + 8:]))
        check_f32(part, pex, ptol, tag + ":partials")
        if filled < nb:
            assert int(_bits(part[filled:]).abs().max()) == 0                                      # blocks without a pixel: exactly 0
        # the wrappers: the same launch, the partials summed by glare_reduce_parts_f32
        for form in ("host", "dev"):
            gzw, ghw = gz0.clone(), torch.full_like(ghF, -7.0)
            if form == "host":
                dM, dt = train_ops.flow_pre_backward_(gzw, z_in, hF, f_off, gl, M32.flatten().tolist(), t32.tolist(), FLOW_EPS, ghw, gf_off)
            else:
                dM, dt = train_ops.flow_pre_backward_(gzw, z_in, hF, f_off, gl, None, None, FLOW_EPS, ghw, gf_off, Mt_dev=Mt_dev)
            assert torch.equal(_bits(gzw), _bits(gz)) and torch.equal(_bits(ghw), _bits(ghF))
            rtol = e_terms.sum(0) + (trips + 8 + _reduce_depth(nb, 12)) * U * terms.abs().sum(0)
            check_f32(torch.cat([dM.flatten(), dt]), terms.sum(0), rtol, tag + ":dMt:" + form)


# ---- 5. groupnorm_backward --------------------------------------------------------------------------------------------------------
# (HW, C, pitch, off): one pixel; fewer pixels than one iteration holds (C = 64: 8 per iteration); 129 = 2 x 64 + 1 at C = 32 (64 per
# iteration); two splits of 150 (C = 128: 16 per iteration, 4x unroll + remainder); 383 = two splits of 192 / 191 at 4 per iteration;
# 16641 = 129 x 129: 130 splits of 129 pixels, the last one EMPTY; C = 2048: one pixel per iteration; a slice of a wider record
GN_BWD_CASES = ((1, 64, 64, 0), (7, 64, 64, 0), (129, 32, 32, 0), (300, 128, 128, 0), (383, 512, 512, 0), (16641, 32, 32, 0),
                (260, 2048, 2048, 0), (300, 64, 128, 32))
GN_VAR_MIN = 1e-4          # the condition of the case: no group's variance near zero (100 x eps), so rstd is set by the data
# seeds at which x ~ N(0.3, 1.5^2) meets it in both formats where a group holds only two values (the larger groups do at any seed)
GN_BWD_SEED = {(1, 64): 1}


def _gn_bwd_inputs(HW, C, pitch, seed):
    """B = 2, the second image at 4x the scale (its upstream gradient at 1 / 4)"""
    g = torch.Generator().manual_seed(seed)
    rec = torch.randn(2, HW, pitch, generator=g) * 1.5 + 0.3
    rec[1] *= 4
    dy = torch.randn(2, HW, C, generator=g)
    dy[1] *= 0.25
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.3
    return _r16(rec), _r16(dy), gamma, beta


def _gn_stats(x64, fsplits):
    """What the forward leaves: per (image, split of the pixels, group) the sums of x and x^2, here in fp64 and rounded to fp32,
    [B][fsplits][32][2]; and mean / rstd taken from those fp32 numbers in double precision, rounded to fp32, as gn_group_stats does"""
    B, HW, C = x64.shape
    cpg = C // 32
    cut = [HW * i // fsplits for i in range(fsplits + 1)]
    xs = [x64[:, cut[i]:cut[i + 1]].reshape(B, cut[i + 1] - cut[i], 32, cpg) for i in range(fsplits)]
    stats = torch.stack([torch.stack([v.sum((1, 3)), (v * v).sum((1, 3))], -1) for v in xs], 1).float()
    S = stats.double().sum(1)
    n = float(HW * cpg)
    m = S[..., 0] / n
    var = (S[..., 1] / n - m * m).clamp_min(0.0)
    return stats.contiguous(), m.float().double(), (1.0 / torch.sqrt(var + _f32(GN_EPS))).float().double(), var


@pytest.mark.parametrize("fsplits", (1, 3))
@pytest.mark.parametrize("swish", (False, True))
@pytest.mark.parametrize("HW,C,pitch,off", GN_BWD_CASES)
def test_groupnorm_backward_per_element(prec, HW, C, pitch, off, swish, fsplits):
    B, cpg = 2, C // 32
    rec, dy, gamma, beta = (t.cuda() for t in _gn_bwd_inputs(HW, C, pitch, GN_BWD_SEED.get((HW, C), HW + C)))
    x64, dy64, ga64, be64 = rec[..., off:off + C].double(), dy.double(), gamma.double(), beta.double()
    stats, mean, rstd, var = _gn_stats(x64, fsplits)
    assert float(var.min()) > GN_VAR_MIN, float(var.min())
    lib = _lib.lib()
    nws = int(lib.glare_groupnorm_backward_workspace_bytes(B, HW, C))
    splits = max(1, min(512, HW // 128))
    assert nws == (B * splits * C * 2 + B * 32 * 2) * 4
    ws = torch.full((nws // 4,), float("nan"), dtype=torch.float32, device="cuda")
    dx = torch.full((B, HW, C), float("nan"), dtype=ops.act_dtype(), device="cuda")
    per_image = torch.full((B, 2, C), float("nan"), dtype=torch.float32, device="cuda")
    check(lib.glare_groupnorm_swish_backward_bf16(ptr(rec), pitch, off, ptr(dy), ptr(stats), fsplits, ptr(gamma), ptr(beta), ptr(dx),
                                                  ptr(per_image), B, HW, C, GN_EPS, int(swish), ptr(ws), nws, stream_handle()),
          "glare_groupnorm_swish_backward_bf16")
    coef = ws[B * splits * C * 2:].view(B, 32, 2)
    sums = train_ops.reduce_parts(per_image)                  # what the wrapper returns: (dbeta, dgamma) = the sum over the images
    if pitch == C:
        dxw, dgw, dbw = train_ops.groupnorm_backward(rec.view(B, 1, HW, C), dy.view(B, 1, HW, C), stats, gamma, beta, swish=swish, eps=GN_EPS)
        assert torch.equal(_bits(dxw.view(B, HW, C)), _bits(dx)) and torch.equal(_bits(dbw), _bits(sums[0]))
        assert torch.equal(_bits(dgw), _bits(sums[1]))
    tag = "gn_bwd:%dx%d:%d:swish%d:f%d" % (HW, C, off, swish, fsplits)
    exact, s1, s2, xh, du = R.groupnorm_backward(x64, dy64, ga64, be64, mean, rstd, swish)
    mu, r = (v.repeat_interleave(cpg, 1).unsqueeze(1) for v in (mean, rstd))
    # xh = (x - mean) * rstd: the difference rounds once on |x| + |mean|, the product once
    e_xh = 2 * U * r * (x64.abs() + mu.abs())
    if swish:
        # u = xh gamma + beta: 2 roundings on its terms.  du = dy * f(u), f = s (1 + u (1 - s)), s = sigmoidf_(u) (__expf):
        # f moves by at most |f'| <= 1/2 per unit of u; at the kernel's u, s carries es, 1 - s the same ABSOLUTE error and its own
        # rounding, then u (1 - s), 1 + ..., s * (...) round once each; the product with dy once
        u = xh * ga64 + be64
        e_u = ga64.abs() * e_xh + 2 * U * ((xh * ga64).abs() + be64.abs())
        s, rel = _sigmoid_rel(u, 2)
        es, k = rel * s, 1.0 + u.abs() * (1.0 - s)
        e_f = 0.5 * e_u + es * k + s * (u.abs() * es + 2 * U * u.abs() * (1.0 - s) + U * k) + U * s * k
        e_du = dy64.abs() * (e_f + U * R.swish_grad(u).abs())
    else:
        e_du = torch.zeros_like(du)
    t2 = du * xh
    e_t2 = e_du * xh.abs() + du.abs() * e_xh + U * t2.abs()
    # the per-image sums: a thread's chain over ceil(per / ppi) pixels, the ppi rows of the block, the splits of the finalize (J
    # interleaved chains and the J - 1 additions that join them)
    ppi = 256 // (C // 8)
    CB = 64 if C % 64 == 0 and 64 % cpg == 0 else C
    J = 256 // CB if CB <= 256 else 1
    per = -(-HW // splits)
    depth = -(-per // ppi) + ppi + -(-splits // J) + J
    A1, A2 = du.abs().sum(1), t2.abs().sum(1)
    sl1, sl2 = e_du.sum(1) + depth * U * A1, e_t2.sum(1) + depth * U * A2
    check_f32(per_image[:, 0].contiguous(), s1, sl1, tag + ":s1")
    check_f32(per_image[:, 1].contiguous(), s2, sl2, tag + ":s2")
    check_f32(sums[0], s1.sum(0), sl1.sum(0) + U * A1.sum(0), tag + ":dbeta")          # one more addition (B = 2)
    check_f32(sums[1], s2.sum(0), sl2.sum(0) + U * A2.sum(0), tag + ":dgamma")
    # the two group coefficients a = sum_c gamma s1 / m, q = sum_c gamma s2 / m: the product with gamma, cpg additions, 1 / m and the
    # product with it (cpg + 3), on the magnitudes of the terms
    m = float(HW * cpg)
    grp = lambda v: v.view(B, 32, cpg).sum(2) / m
    a, q = grp(s1 * ga64), grp(s2 * ga64)
    e_a, e_q = grp(sl1 * ga64.abs() + (cpg + 3) * U * A1 * ga64.abs()), grp(sl2 * ga64.abs() + (cpg + 3) * U * A2 * ga64.abs())
    check_f32(coef[..., 0].contiguous(), a, e_a, tag + ":coef_a")
    check_f32(coef[..., 1].contiguous(), q, e_q, tag + ":coef_q")
    # dx = rstd * (du gamma - a - xh q): the two products round once each on top of what they read, the two subtractions on the three
    # terms, the product with rstd; the coefficients' own errors enter as rstd (e_a + |xh| e_q)
    a, q, e_a, e_q = (v.repeat_interleave(cpg, 1).unsqueeze(1) for v in (a, q, e_a, e_q))
    v1, v3 = du * ga64, xh * q
    e1 = ga64.abs() * e_du + U * v1.abs()
    e3 = e_xh * q.abs() + xh.abs() * e_q + U * v3.abs()
    slack = r * (e1 + e_a + e3 + 2 * U * (v1.abs() + a.abs() + v3.abs())) + U * exact.abs()
    assert_rounded(dx, exact, slack, tag + ":dx")


# ---- 6. mix_backward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("host", "dev"))
@pytest.mark.parametrize("want_ga", (False, True))
@pytest.mark.parametrize("w", (-0.6, 0.3, 5.0))
@pytest.mark.parametrize("n", (8, 2056, 1048584))
def test_mix_backward_per_element(prec, n, w, want_ga, form):
    """1, 257 and 131 073 chunks of 8: the last is more than 512 x 256, a second trip"""
    gen = torch.Generator().manual_seed(n % 1000 + int(w * 10) + 50)
    g, a, b = (_r16(torch.randn(n, generator=gen)).cuda() for _ in range(3))
    wl = torch.tensor(w, dtype=torch.float32, device="cuda") if form == "dev" else w
    ga, gb, dw = train_ops.mix_backward(g, a, b, wl, want_ga=want_ga)
    w64 = torch.tensor(_f32(w), dtype=torch.float64, device="cuda")
    ega, egb, edw = R.mix_backward(g.double(), a.double(), b.double(), w64)
    s, rel = _sigmoid_rel(w64, 0)                                    # expf of the fp32 logit, on the host or on the device
    tag = "mix_bwd:%d:%g:%s" % (n, w, form)
    # ga = s g: s's error and the product; gb = (1 - s) g: 1 - s carries s's ABSOLUTE error and its own rounding, then the product
    if want_ga:
        assert_rounded(ga, ega, ega.abs() * (rel + U), tag + ":ga")
    else:
        assert ga is None
    assert_rounded(gb, egb, g.double().abs() * (s * rel + 2 * U * (1.0 - s)), tag + ":gb")
    # dw = s (1 - s) sum g (a - b).  A term: the difference and the product round once each (2); the sum: 8 additions per trip and
    # thread, 6 shuffles, 3 over the four waves (8 trips + 9), then the chain of glare_reduce_parts_f32 over the blocks.  The host form
    # multiplies by s (1 - s) once, after the sum; the device form multiplies every block's partial before it: one rounding on every
    # term's path either way (1).  s (1 - s) itself: s's error through |1 - 2 s|, the rounding of 1 - s and of the product
    n8 = n // 8
    blocks = max(1, min(512, -(-n8 // 256)))
    trips = -(-n8 // (blocks * 256))
    assert trips == (2 if n == 1048584 else 1)
    count = 2 + 8 * trips + 9 + _reduce_depth(blocks, 1) + 1
    rel_scale = (1.0 - 2.0 * s).abs() * rel / (1.0 - s) + 2 * U
    mag = (g.double() * (a.double() - b.double())).abs().sum()
    check_f32(dw, edw.reshape(1), (s * (1.0 - s) * mag * (count * U + rel_scale)).reshape(1), tag + ":dw")


def test_mix_backward_rejects_a_ragged_length(prec):
    g, a, b, gb = (torch.zeros(16, dtype=ops.act_dtype(), device="cuda") for _ in range(4))
    dw, ws = torch.zeros(1, device="cuda"), torch.zeros(512, device="cuda")
    lib = _lib.lib()
    assert lib.glare_mix_backward_bf16(ptr(g), ptr(a), ptr(b), None, ptr(gb), 12, 0.3, ptr(dw), ptr(ws), 2048, stream_handle()) == _lib.ERR_INVALID
    assert lib.glare_mix_backward_dev_bf16(ptr(g), ptr(a), ptr(b), None, ptr(gb), 12, ptr(dw), ptr(dw), ptr(ws), 2048,
                                           stream_handle()) == _lib.ERR_INVALID


# ---- 7. mean_rescale_backward -----------------------------------------------------------------------------------------------------
RESCALE_BWD_BLOCKS = 512


@pytest.mark.parametrize("n", (8, 13, 4104, 4099, 1048584))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("whole", (False, True))
def test_mean_rescale_backward_per_block_and_per_element(prec, whole, B, n):
    """n % 8 == 0: the vector path (8 elements per thread and trip); 13 and 4099: the scalar path; 1 048 584 = 131 073 vectors
    > 512 x 256: a second trip.  xw in [0.5, 1.5]: sum xw = sum |xw|, as well conditioned as a sum can be."""
    gen = torch.Generator().manual_seed(n % 1000 + B)
    g = _r16(torch.randn(B, n, generator=gen)).cuda()
    h = _r16(torch.randn(B, n, generator=gen) + 0.2 + 0.1 * torch.arange(B).view(B, 1)).cuda()
    xw = (torch.rand(B, n, generator=gen) + 0.5).cuda()
    assert float(xw.min()) >= 0.5 and float(xw.max()) <= 1.5
    lib = _lib.lib()
    nws = int(lib.glare_mean_rescale_backward_workspace_bytes(B, n))
    assert nws == (B * RESCALE_BWD_BLOCKS * 3 + B * 3) * 4

    def run(g_, h_, xw_):
        ws = torch.full((nws // 4,), float("nan"), dtype=torch.float32, device="cuda")
        gh, gxw = torch.full_like(h_, float("nan")), torch.full_like(xw_, float("nan"))
        check(lib.glare_mean_rescale_backward_bf16(ptr(g_), ptr(h_), ptr(xw_), ptr(gh), ptr(gxw), B, n, int(whole), ptr(ws), nws,
                                                   stream_handle()), "glare_mean_rescale_backward_bf16")
        return gh, gxw, ws[:B * RESCALE_BWD_BLOCKS * 3].view(B, RESCALE_BWD_BLOCKS, 3), ws[B * RESCALE_BWD_BLOCKS * 3:].view(B, 3)

    gh, gxw, part, coef = run(g, h, xw)
    ghw, gxww = train_ops.mean_rescale_backward(g, h, xw, whole)
    assert torch.equal(_bits(ghw), _bits(gh)) and torch.equal(_bits(gxww), _bits(gxw))
    tag = "rescale_bwd:%d:%d:%d" % (n, B, whole)
    g64, h64, x64 = g.double(), h.double(), xw.double()
    # partial[b][blk] = (D, Sh, Sx) of the slice: block blk owns the vectors (or, n % 8 != 0, the elements) blk * 256 + t + k * 512 * 256.
    # Additions behind a partial: per trip and thread 8 (vector path) or 1, 6 shuffles, 3 over the four waves; D's products round once more
    vec = n % 8 == 0
    items = n // 8 if vec else n
    trips = -(-items // (RESCALE_BWD_BLOCKS * 256))
    assert trips == (2 if n == 1048584 else 1)
    adds = (8 if vec else 1) * trips + 9
    block_of = ((torch.arange(n, device="cuda") // (8 if vec else 1)) // 256) % RESCALE_BWD_BLOCKS
    e_sum = []
    for k, (v, extra) in enumerate(((g64 * x64, 1), (h64, 0), (x64, 0))):
        pex = torch.stack([_block_sum(v[b].unsqueeze(1), block_of, RESCALE_BWD_BLOCKS)[:, 0] for b in range(B)])
        ptol = (adds + extra) * U * torch.stack([_block_sum(v[b].abs().unsqueeze(1), block_of, RESCALE_BWD_BLOCKS)[:, 0] for b in range(B)])
        check_f32(part[..., k].contiguous(), pex, ptol, tag + ":partials%d" % k)
        e_sum.append(ptol.sum(1))
    # coef[b] = (D / Sx, r = Sh / Sx, D Sh / Sx^2): the partials added and divided in double precision, rounded to fp32 once; the
    # sums' errors (of the sample, or of the batch) enter through the quotients' derivatives
    e_D, e_Sh, e_Sx = ((v.sum().expand(B) if whole else v) for v in e_sum)
    D, Sh, Sx = R.mean_rescale_sums(g64, h64, x64, whole)
    c0, c1, c2 = D / Sx, Sh / Sx, D * Sh / (Sx * Sx)
    e0 = e_D / Sx + D.abs() * e_Sx / Sx ** 2 + U * c0.abs()
    e1 = e_Sh / Sx + Sh.abs() * e_Sx / Sx ** 2 + U * c1.abs()
    e2 = (e_D * Sh.abs() + D.abs() * e_Sh) / Sx ** 2 + 2 * (D * Sh).abs() * e_Sx / Sx ** 3 + U * c2.abs()
    check_f32(coef.contiguous(), torch.stack([c0, c1, c2], 1), torch.stack([e0, e1, e2], 1), tag + ":coef")
    # gh = g + c0: one rounding on |g| + |c0|; gxw = g c1 - c2: the product and the difference
    egh, egxw = R.mean_rescale_backward(g64, h64, x64, whole)
    assert_rounded(gh, egh, e0[:, None] + U * (g64.abs() + c0.abs()[:, None]), tag + ":gh")
    check_f32(gxw, egxw, g64.abs() * e1[:, None] + e2[:, None] + 2 * U * ((g64 * c1[:, None]).abs() + c2.abs()[:, None]), tag + ":gxw")
    if B == 3 and not whole:          # per-sample means: a sample's gradients come from its own sums only
        g3, h3, x3 = g.clone(), h.clone(), xw.clone()
        g3[1], h3[1], x3[1] = -g3[1], _r16(h3[1].float() * 3 + 1), x3[1] * 1.25
        gh3, gxw3, _, _ = run(g3, h3, x3)
        for b in (0, 2):
            assert torch.equal(_bits(gh3[b]), _bits(gh[b])) and torch.equal(_bits(gxw3[b]), _bits(gxw[b]))
        assert not torch.equal(_bits(gh3[1]), _bits(gh[1]))


# ---- 8. act_backward_ -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (3, 64))
@pytest.mark.parametrize("act", ("relu", "sigmoid"))
@pytest.mark.parametrize("y32", (False, True))
@pytest.mark.parametrize("g32", (False, True))
def test_act_backward_per_element(prec, g32, y32, act, C):
    """g and y in either type with independent pitches and offsets; y holds +0, -0 and the smallest positive 16-bit value (a
    subnormal: 2^-133 in bf16 is one in fp32 as well).  The references are computed on the CPU."""
    m, emin = _fmt()
    tiny = 2.0 ** (emin - m)
    gen = torch.Generator().manual_seed(C + 2 * g32 + y32)
    pixels = 37                                                     # 37 x 64 elements: ten blocks, the last one ragged
    for (gp, go), (yp, yo) in (((72, 8), (64, 0)), ((64, 0), (72, 8))):
        g0 = torch.randn(pixels, gp, generator=gen)
        y0 = torch.randn(pixels, yp, generator=gen) if act == "relu" else torch.rand(pixels, yp, generator=gen)
        y0[0, yo:yo + 3] = torch.tensor([0.0, -0.0, tiny])
        g0 = g0 if g32 else _r16(g0)
        y0 = y0 if y32 else _r16(y0)
        assert float(y0[0, yo + 2]) == tiny and math.copysign(1.0, float(y0[0, yo + 1])) == -1.0
        gd = g0.cuda()
        assert train_ops.act_backward_(gd, y0.cuda(), act, C=C, g_off=go, y_off=yo) is gd
        got = gd.cpu()
        assert torch.equal(_bits(got[:, :go]), _bits(g0[:, :go])) and torch.equal(_bits(got[:, go + C:]), _bits(g0[:, go + C:]))
        gs, ys, out = g0[:, go:go + C], y0[:, yo:yo + C], got[:, go:go + C].contiguous()
        tag = "act_bwd:%s:g%d:y%d:%d:%d" % (act, 32 if g32 else 16, 32 if y32 else 16, C, gp)
        exact = R.act_backward(gs.double(), ys.double(), act)
        if act == "relu":          # a selection: the same bits, a +0 where y <= 0
            assert torch.equal(_bits(out), _bits(exact.to(gs.dtype))), tag
            assert float(out[0, 2]) == float(gs[0, 2]) and int(_bits(out)[0, 0]) == 0 and int(_bits(out)[0, 1]) == 0
        elif g32:                  # g * y * (1 - y): two roundings, each at worst half the spacing of the fp32 subnormals (2^-150) where
            #                        the product falls below 2^-126 (y = 2^-133 in bf16) ...
            check_f32(out, exact, 2 * U * exact.abs() + 2 * 2.0 ** -150, tag)
        else:                      # ... plus the store (ulp16 has the 16-bit format's own floor)
            assert_rounded(out, exact, 2 * U * exact.abs() + 2 * 2.0 ** -150, tag)
