"""GPU: the patch discriminator's kernels (csrc/conv4x4.hip, csrc/disc_ops.hip) PER ELEMENT against fp64 (tests/disc_oracle.py), in both
16-bit precisions, at the shapes where their index arithmetic changes regime: odd sides (the stride-2 floor, the right / bottom padding),
a 1 x 1 output, channel counts that are no multiple of the 32-channel MFMA step (72), the dense-k forms (3 input channels, 1 output
channel) and both filter-row tiles (16 and 64).  Failed on the parent commit: the wrappers did not exist.

Bounds, as tests/test_gpu_backward_edges.py states them (fp64_bounds.py):
    16-bit outputs   |got - exact| <= 0.5 ulp16(exact) + slack            fp32 outputs   |got - exact| <= slack
with slack counted from the kernel's own expression.  Operands are 16-bit values on both sides (the filter pack and the im2col round
to the 16-bit format: exact on such values), so every product of an MFMA is exact in fp32 and only its accumulation rounds:
    a sum of K products on the MFMA    2 U (K + 1) sum |terms|     (K counts the zero padding the kernel multiplies as well; the MFMA's
                                       internal additions are not specified to round to nearest: one ulp = 2 U each, not half)
    bias, LeakyReLU                    + 2 U (one addition, one product; the activation is 1-Lipschitz, so an argument on the other
                                       side of the kink within its error stays inside the bound)
BatchNorm and the hinge sums: counted step by step in disc_oracle.bn_forward_64 / bn_backward_64 and next to the calls below.
Every kernel is launched twice on the same input and must agree bit for bit.

Measured / bound on the MI355X (largest over the cases; bf16 | fp16): see DESIGN.md section 9."""
import pytest
import torch

import disc_oracle as R
from fp64_bounds import U, _bits, _f32, _r16, _tag, assert_rounded
from glare_amd import _lib, ops, train_ops as T
from tolerances import within

pytestmark = pytest.mark.gpu

SHAPES = ((2, 2), (5, 7), (6, 10), (9, 8))
CHANNELS = ((3, 64), (64, 128), (72, 8), (512, 1))
GEOMETRY = [(H, W, s) for H, W in SHAPES for s in (1, 2) if not ((H, W) == (2, 2) and s == 2)]        # 2 x 2: stride 1 only (a 1 x 1 output)


@pytest.fixture(params=("bf16", "fp16"))
def prec(request):
    with ops.use_precision(request.param):
        yield request.param


def _ratio(err, bound):
    return torch.where(err == 0, torch.zeros_like(err), err / bound)


def check_f32(got32, exact64, tol64, tag):
    assert got32.dtype == torch.float32 and tuple(got32.shape) == tuple(exact64.shape), (got32.dtype, got32.shape, exact64.shape)
    return within(float(_ratio((got32.double().cpu() - exact64).abs(), tol64).max()), 1.0, _tag(tag))


def check_r16(got16, exact64, slack64, tag):
    return assert_rounded(got16.cpu(), exact64, slack64, tag)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rup(a, b):
    return (a + b - 1) // b * b


def _conv_case(H, W, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = _r16(torch.randn(2, H, W, cin, generator=g)).float()             # 16-bit values; layer 1 reads them as fp32
    w = _r16(torch.randn(cout, cin, 4, 4, generator=g) * 0.25).float()
    b = torch.randn(cout, generator=g)
    return x, w, b, g


def _k_forward(cin):
    """products behind one forward output, zero padding included: 16 taps x channels rounded up to the 32-wide MFMA step (dense k: 16 Cin
    rounded up to 32)"""
    return _rup(16 * cin, 32) if cin < 8 else 16 * _rup(cin, 32)


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("H,W,stride", GEOMETRY)
def test_conv4x4_forward_per_element(prec, H, W, cin, cout, stride):
    x, w, b, _ = _conv_case(H, W, cin, cout, 1000 * H + 10 * W + cin + stride)
    xd = (x if cin == 3 else _r16(x)).cuda()
    wd, bd = w.cuda(), b.cuda()
    K = _k_forward(cin)
    for bias, act in ((False, False), (True, False), (False, True), (True, True)):
        ref = R.conv4x4_64(x, w, b if bias else None, None, stride)
        exact = R.lrelu64(ref["y"]) if act else ref["y"]
        slack = 2 * U * (K + 1) * ref["ymag"] + 2 * U * ref["ymag"]
        tag = "fwd:%dx%d:%d-%d:s%d:b%d:a%d" % (H, W, cin, cout, stride, bias, act)
        y = T.conv4x4_forward(xd, wd, bd if bias else None, stride=stride, lrelu=act)
        assert tuple(y.shape) == (2, T.conv4x4_out(H, stride), T.conv4x4_out(W, stride), cout)
        check_r16(y, exact, slack, tag)
        assert _same_bits(y, T.conv4x4_forward(xd, wd, bd if bias else None, stride=stride, lrelu=act)), tag
        if not act:       # the fp32 store (the logits' form): the same accumulator, no 16-bit rounding
            y32 = T.conv4x4_forward(xd, wd, bd if bias else None, stride=stride, out_f32=True)
            check_f32(y32, exact, slack, tag + ":f32")
            assert _same_bits(y32, T.conv4x4_forward(xd, wd, bd if bias else None, stride=stride, out_f32=True)), tag


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("H,W,stride", GEOMETRY)
def test_conv4x4_gradients_per_element(prec, H, W, cin, cout, stride):
    x, w, b, g = _conv_case(H, W, cin, cout, 2000 * H + 10 * W + cin + stride)
    OH, OW = T.conv4x4_out(H, stride), T.conv4x4_out(W, stride)
    gy = _r16(torch.randn(2, OH, OW, cout, generator=g)).float()
    ref = R.conv4x4_64(x, w, b, gy, stride)
    xd = (x if cin == 3 else _r16(x)).cuda()
    wd = w.cuda()
    pitch = _rup(cout, 8)                                  # the gradient enters with a channel pitch that is a multiple of 8 (extra channels 0)
    g16 = torch.zeros(2, OH, OW, pitch, dtype=ops.act_dtype())
    g16[..., :cout] = _r16(gy)
    g16 = g16.cuda()
    tag = "%dx%d:%d-%d:s%d" % (H, W, cin, cout, stride)

    # data gradient: 16 taps (stride 2, parity classes: 4) x the gradient's channels rounded up to 32; dense k for a 1-channel gradient
    taps = 16 if (stride == 1 or pitch < 8 or cout < 8) else 4
    K = _rup(16 * cout, 32) if cout < 8 else taps * _rup(pitch, 32)
    slack = 2 * U * (K + 1) * ref["dxmag"]
    dx = T.conv4x4_dgrad(g16, wd, (2, H, W, cin), stride=stride, out_f32=cin == 3)
    if cin == 3:                                           # d xrec: fp32
        check_f32(dx, ref["dx"], slack, "dgrad:" + tag)
    else:
        check_r16(dx, ref["dx"], slack, "dgrad:" + tag)
    assert _same_bits(dx, T.conv4x4_dgrad(g16, wd, (2, H, W, cin), stride=stride, out_f32=cin == 3)), tag

    # weight gradient: K = the pixel axis rounded up to the GEMM's 64 (one split at these sizes), then no further sum
    P = 2 * OH * OW
    Kp = _rup(P, 64)
    dwb = T.conv4x4_weight_grad(xd, g16, cout, stride)
    assert tuple(dwb.shape) == (cout, 16 * cin + 1)
    check_f32(dwb[:, :-1].contiguous().view(cout, cin, 4, 4), ref["dw"], 2 * U * (Kp + 1) * ref["dwmag"], "wgrad:" + tag)
    check_f32(dwb[:, -1].contiguous(), ref["db"], 2 * U * (Kp + 1) * ref["dbmag"], "bgrad:" + tag)
    assert _same_bits(dwb.contiguous(), T.conv4x4_weight_grad(xd, g16, cout, stride).contiguous()), tag


def test_conv4x4_refuses_what_it_cannot_index(prec):
    x = torch.zeros(1, 1, 1, 8, dtype=ops.act_dtype(), device="cuda")
    with pytest.raises(AssertionError):
        T.conv4x4_forward(x, torch.zeros(8, 8, 4, 4, device="cuda"), stride=1)          # 1 x 1 input: no output pixel
    lib = _lib.lib()
    # 2^31 pixels: reported, nothing launched (the pointers are never read)
    rc = lib.glare_conv4x4_forward_bf16(x.data_ptr(), 0, 8, x.data_ptr(), None, x.data_ptr(), 0, 8, 1 << 15, 1 << 8, 1 << 8, 8, 8, 1, 0, None)
    assert rc == _lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("n", (1, 13, 4099))
def test_lrelu_backward_per_element(prec, n):
    g = torch.Generator().manual_seed(n)
    gy = _r16(torch.randn(n, 8, generator=g))
    y = _r16(torch.randn(n, 8, generator=g))
    y.view(-1)[::5] = 0.0                                   # at the kink: the slope side, as torch's leaky_relu_backward (x > 0 ? 1 : slope)
    out = T.lrelu_backward(gy.cuda(), y.cuda())
    exact = torch.where(y.double() > 0, gy.double(), R.SLOPE * gy.double())
    check_r16(out, exact, U * exact.abs(), "lrelu_bwd:%d" % n)
    assert torch.equal(_bits(out.cpu())[y > 0], _bits(gy)[y > 0])                        # untouched where the activation passed
    assert _same_bits(out, T.lrelu_backward(gy.cuda(), y.cuda()))


BN_SHAPES = ((2, 5, 7, 128), (1, 1, 3, 8), (4, 6, 6, 512))


@pytest.mark.parametrize("groups", (1, 2))
@pytest.mark.parametrize("B,H,W,C", BN_SHAPES)
def test_batchnorm_per_element(prec, B, H, W, C, groups):
    g = torch.Generator().manual_seed(B * 100 + C + groups)
    x = torch.randn(B, H, W, C, generator=g) * 1.5 + 0.3
    x[..., 3] = 0.75                                        # a channel of constant input: variance 0
    x = _r16(x)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dy = _r16(torch.randn(B, H, W, C, generator=g))
    xd, dyd, gd, bd = x.cuda(), dy.cuda(), gamma.cuda(), beta.cuda()
    tag = "%dx%dx%dx%d:g%d" % (B, H, W, C, groups)
    if B % groups:
        with pytest.raises(AssertionError):                 # one image is not two groups
            T.batchnorm_forward(xd, gd, bd, groups=groups)
        return
    eps, mom = _f32(1e-5), _f32(0.1)
    n = B // groups * H * W
    (y64, mean64, var64, rstd64), (e_y, e_mean, e_var, e_rstd) = R.bn_forward_64(x, gamma, beta, groups, eps)

    def run():
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        nbt = torch.zeros((), dtype=torch.int64, device="cuda")
        for _ in range(2):
            y, saved = T.batchnorm_forward(xd, gd, bd, groups=groups, lrelu=True, eps=1e-5, momentum=0.1, running_mean=rm, running_var=rv,
                                           num_batches_tracked=nbt)
        return y, saved, rm, rv, nbt

    y, saved, rm, rv, nbt = run()
    check_r16(y.view(groups, -1, C), y64, e_y, "bn:y:" + tag)
    check_f32(saved[:, 0].contiguous(), mean64, e_mean, "bn:mean:" + tag)
    check_f32(saved[:, 1].contiguous(), rstd64, e_rstd, "bn:rstd:" + tag)
    assert float(var64[:, 3].max()) == 0.0 and bool(torch.isfinite(y.float()).all())
    # running statistics after two calls = 2 x groups momentum updates in (call, group) order, from (0, 1):
    #   r' = (1 - m) r + m s   three roundings on the two terms + the rounding of 1 - m (U |r|): 4 U (|r| + |m s|), and 0.9 e(r) + m e(s);
    #   s = mean, or var n / (n - 1): e_var n / (n - 1) + 2 U s
    unb = var64 * n / max(n - 1, 1)
    e_unb = e_var * n / max(n - 1, 1) + 2 * U * unb
    r_m, r_v = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    e_m, e_v = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for _ in range(2):
        for k in range(groups):
            e_m = (1 - mom) * e_m + mom * e_mean[k] + 4 * U * (r_m.abs() + (mom * mean64[k]).abs())
            e_v = (1 - mom) * e_v + mom * e_unb[k] + 4 * U * (r_v.abs() + (mom * unb[k]).abs())
            r_m = (1 - mom) * r_m + mom * mean64[k]
            r_v = (1 - mom) * r_v + mom * unb[k]
    check_f32(rm, r_m, e_m, "bn:running_mean:" + tag)
    check_f32(rv, r_v, e_v, "bn:running_var:" + tag)
    assert int(nbt) == 2 * groups
    # what nn.BatchNorm2d leaves after the same calls (fp32, per group as separate calls): the same numbers to its own rounding
    bn = torch.nn.BatchNorm2d(C).train()
    for _ in range(2):
        for k in range(groups):
            bn(x.float().view(groups, -1, H, W, C)[k].permute(0, 3, 1, 2))
    assert int(bn.num_batches_tracked) == int(nbt)
    check_f32(rv, bn.running_var.double(), 2 * e_v + 1e-30, "bn:running_var vs nn:" + tag)

    (dx64, dg64, db64), (e_dx, e_dg, e_db) = R.bn_backward_64(x, dy, saved, gamma, beta, groups)
    dx, dgamma, dbeta = T.batchnorm_backward(xd, dyd, saved, gd, bd, groups=groups, lrelu=True)
    check_r16(dx.view(groups, -1, C), dx64, e_dx, "bn:dx:" + tag)
    check_f32(dgamma, dg64, e_dg, "bn:dgamma:" + tag)
    check_f32(dbeta, db64, e_db, "bn:dbeta:" + tag)

    y2, saved2, rm2, rv2, _ = run()
    dx2, dgamma2, dbeta2 = T.batchnorm_backward(xd, dyd, saved, gd, bd, groups=groups, lrelu=True)
    for a, b in ((y, y2), (saved, saved2), (rm, rm2), (rv, rv2), (dx, dx2), (dgamma, dgamma2), (dbeta, dbeta2)):
        assert _same_bits(a, b), tag


def test_batchnorm_groups_are_separate_calls(prec):
    """Two groups in one launch = the two halves in two launches, bit for bit (outputs, saved statistics, running statistics, dx);
    dgamma / dbeta = the two calls' sum."""
    g = torch.Generator().manual_seed(5)
    x = _r16(torch.randn(4, 5, 7, 128, generator=g)).cuda()
    dy = _r16(torch.randn(4, 5, 7, 128, generator=g)).cuda()
    gamma, beta = torch.randn(128, generator=g).cuda(), torch.randn(128, generator=g).cuda()
    bufs = lambda: (torch.zeros(128, device="cuda"), torch.ones(128, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda"))
    rm, rv, nbt = bufs()
    y, saved = T.batchnorm_forward(x, gamma, beta, groups=2, running_mean=rm, running_var=rv, num_batches_tracked=nbt)
    dx, dga, dbe = T.batchnorm_backward(x, dy, saved, gamma, beta, groups=2)
    rm1, rv1, nbt1 = bufs()
    parts = []
    for k in range(2):
        xk, dyk = x[2 * k:2 * k + 2].contiguous(), dy[2 * k:2 * k + 2].contiguous()
        yk, sk = T.batchnorm_forward(xk, gamma, beta, groups=1, running_mean=rm1, running_var=rv1, num_batches_tracked=nbt1)
        parts.append((yk, sk) + T.batchnorm_backward(xk, dyk, sk, gamma, beta, groups=1))
    assert _same_bits(y, torch.cat([p[0] for p in parts])) and _same_bits(saved, torch.cat([p[1] for p in parts]))
    assert _same_bits(dx, torch.cat([p[2] for p in parts]))
    assert _same_bits(rm, rm1) and _same_bits(rv, rv1) and int(nbt) == int(nbt1) == 2
    assert _same_bits(dga, parts[0][3] + parts[1][3]) and _same_bits(dbe, parts[0][4] + parts[1][4])


@pytest.mark.parametrize("n", (1, 13, 4099))
def test_hinge_reductions(n):
    """Values on both sides of each kink, exactly at it (+-1) and next to it.  t = 1 -+ x rounds once, the sum of n terms n times, the
    division once: (n + 2) U sum |t| / n.  The indicator of the gradient is exact (a rounded difference keeps its sign) and -+1 / n is
    one rounding of 1 / n."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 2
    x[0::7] = 1.0
    x[3::7] = -1.0
    if n > 6:
        x[5], x[6] = 1.0 + 2.0 ** -23, -1.0 + 2.0 ** -24
    xd, x64 = x.cuda(), x.double()
    for mode, t64, ind in (("real", (1 - x64).clamp_min(0), -(x64 < 1).double()), ("fake", (1 + x64).clamp_min(0), (x64 > -1).double()),
                           ("generator", -x64, -torch.ones_like(x64))):
        loss, grad = T.hinge_loss(xd, mode)
        mag = (1 + x64.abs()).sum() if mode != "generator" else x64.abs().sum()
        print("hinge %s n=%d: loss %.9g exact %.9g" % (mode, n, float(loss), float(t64.mean())))
        check_f32(loss, t64.mean().view(1), (n + 2) * U * mag / n, "hinge:%s:%d" % (mode, n))
        check_f32(grad, ind / n, U * ind.abs() / n, "hinge:%s:%d:grad" % (mode, n))
        assert bool((grad[x == (1.0 if mode == "real" else -1.0)] == 0).all()) or mode == "generator"       # relu'(0) = 0, as torch
        loss2, grad2 = T.hinge_loss(xd, mode)
        assert _same_bits(loss, loss2) and _same_bits(grad, grad2)
