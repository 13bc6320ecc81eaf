"""GPU: the LPIPS head (forward and backward) and the image affine map (csrc/lpips_ops.hip) PER ELEMENT against fp64
(tests/lpips_fp64.py), in both 16-bit precisions.  Failed on the parent commit: train_ops.lpips_head / image_affine did not exist.

Bounds, as tests/test_gpu_backward_edges.py states them (fp64_bounds.py):
    the stored gradient   |got - exact| <= 0.5 ulp16(exact) + slack            the per-image value (fp32)   |got - exact| <= tol
slack / tol counted from the kernel's own expression in lpips_fp64.py's docstring; none is taken from a measurement of the kernel.

Shapes: every wave-per-pixel split (C = 64 .. 512: 8 .. 64 lanes per pixel); 1 x 1 (one pixel), 2 x 2 (fewer pixels than a wave holds),
5 x 7 (a tail that fills no workgroup), 33 x 31 (more than one workgroup per image); B = 3 with a different g[i] per image.  Every case
holds one all-zero pixel in a (gradient exactly 0 there), one in b and one pixel with a single non-zero channel, one per image.
Measured / bound on the MI355X (largest over the cases; bf16 | fp16): gradient 0.9995 | 0.99997 (a correctly rounded store uses up to 1.0),
value 0.032 | 0.036, affine 0.993, its backward 0.987; DESIGN.md section 9."""
import pytest
import torch

import lpips_fp64 as R
from fp64_bounds import _bits, _f32, _r16, _tag, assert_rounded
from glare_amd import _lib, ops, train_ops as T
from tolerances import within

pytestmark = pytest.mark.gpu

CHANNELS = (64, 128, 256, 512)
SIDES = ((1, 1), (2, 2), (5, 7), (33, 31))
EPS = _f32(T.LPIPS_EPS)


@pytest.fixture(params=("bf16", "fp16"))
def prec(request):
    with ops.use_precision(request.param):
        yield request.param


def _check_f32(got32, exact64, tol64, tag):
    assert got32.dtype == torch.float32 and tuple(got32.shape) == tuple(exact64.shape)
    err = (got32.double().cpu() - exact64).abs()
    return within(float(torch.where(err == 0, torch.zeros_like(err), err / tol64).max()), 1.0, _tag(tag))


def _features(B, H, W, C, seed, mag=1.0):
    """ReLU-like 16-bit feature maps with the three edge pixels, one per image (in turn over the pixels when B * H * W allows)."""
    g = torch.Generator().manual_seed(seed)
    top = 1.0 if mag > 1 else 1e9                            # at the top of the range: relu(randn) cut at 1, so that nothing rounds to inf
    a = _r16(torch.relu(torch.randn(B, H, W, C, generator=g)).clamp_max(top) * mag)
    b = _r16(torch.relu(torch.randn(B, H, W, C, generator=g)).clamp_max(top) * mag)
    w = torch.rand(C, generator=g)
    a[0, H - 1, W - 1] = 0                                   # all-zero pixel in a
    b[1 % B, 0, W // 2] = 0                                  # all-zero pixel in b
    one = a[2 % B, H // 2, 0].clone()
    a[2 % B, H // 2, 0] = 0
    a[2 % B, H // 2, 0, C - 3] = one.max().clamp_min(_r16(torch.tensor(mag)))      # a single non-zero channel
    return a, b, w


def _run(a, b, w, g, tag):
    ad, bd, wd, gd = a.cuda(), b.cuda(), w.cuda(), g.cuda()
    ref = R.head64(a, b, w, g, EPS)
    out = T.lpips_head(ad, bd, wd)
    da = T.lpips_head_backward(ad, bd, wd, gd)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(da.float()).all()), tag
    r_out = _check_f32(out, ref["out"], ref["out_tol"], "head:" + tag)
    r_da = assert_rounded(da.cpu(), ref["da"], ref["da_slack"], "head_bwd:" + tag)
    print("lpips head %s %s: value measured / bound %.3g, gradient %.3g" % (ops.precision(), tag, r_out, r_da))
    zero = a.double().abs().sum(-1) == 0
    assert bool(zero.any()) and bool((_bits(da.cpu())[zero] == 0).all()), tag         # gradient of the zero pixel: exactly +0
    assert torch.equal(_bits(out), _bits(T.lpips_head(ad, bd, wd))), tag               # two launches, the same bits
    assert torch.equal(_bits(da), _bits(T.lpips_head_backward(ad, bd, wd, gd))), tag
    return out, da


@pytest.mark.parametrize("H,W", SIDES)
@pytest.mark.parametrize("C", CHANNELS)
def test_head_per_element(prec, C, H, W):
    a, b, w = _features(3, H, W, C, 100 * C + 10 * H + W)
    g = torch.tensor([0.7, -1.3, 2.1])                       # a different upstream gradient per image
    out, da = _run(a, b, w, g, "%dx%dx%d" % (H, W, C))
    # the image index: image i's gradient scales with g[i] alone
    g2 = torch.tensor([0.7, 2.6, 2.1])
    da2 = T.lpips_head_backward(a.cuda(), b.cuda(), w.cuda(), g2.cuda())
    assert torch.equal(_bits(da2[0]), _bits(da[0])) and torch.equal(_bits(da2[2]), _bits(da[2]))
    assert not torch.equal(_bits(da2[1]), _bits(da[1]))


@pytest.mark.parametrize("mag", (1e-4, 65504.0))
@pytest.mark.parametrize("C", (64, 512))
def test_head_at_the_ends_of_the_fp16_range(prec, C, mag):
    """Features at 1e-4 (fp16 subnormals among them) and at the largest fp16-safe magnitude: the sum of squares, the norm and the divisions
    are fp32 (65504^2 x 512 = 2.2e12; 1e-8 x 64)."""
    a, b, w = _features(3, 5, 7, C, 7 * C + int(mag > 1), mag=mag)
    _run(a, b, w, torch.tensor([1.0, -0.5, 2.0]), "5x7x%d:mag%g" % (C, mag))


@pytest.mark.parametrize("H,W", ((5, 7), (33, 31)))
@pytest.mark.parametrize("C", (64, 512))
def test_head_gradient_is_rounded_once_after_the_loss_scale(prec, C, H, W):
    """g carries the fp16 loss scale 2^16 (and 1 / B): the product with 1 / HW is formed in fp32 and rounded to 16 bits once -- the same
    0.5 ulp16 + slack as unscaled.  Rounded before the scale, 2 w d / (HW na) at HW ~ 1e3 sits among fp16's subnormals."""
    a, b, w = _features(3, H, W, C, 9 * C + H)
    _run(a, b, w, torch.tensor([1.0, 0.5, 0.25]) * (65536.0 / 3), "%dx%dx%d:scale" % (H, W, C))


def test_head_error_codes(prec):
    lib = _lib.lib()
    B, HW, C = 2, 35, 64
    x = torch.zeros(B, 5, 7, C, dtype=ops.act_dtype(), device="cuda")
    w = torch.ones(C, device="cuda")
    out = torch.zeros(B, device="cuda")
    need = lib.glare_lpips_head_workspace_bytes(B, HW, C)
    assert need >= B * 4
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    assert lib.glare_lpips_head_bf16(p(x), p(x), p(w), B, HW, C, 1e-10, p(out), p(ws), need, None) == 0
    assert lib.glare_lpips_head_bf16(p(x), p(x), p(w), B, HW, C, 1e-10, p(out), p(ws), need - 1, None) == _lib.ERR_WORKSPACE
    assert lib.glare_lpips_head_bf16(p(x), p(x), p(w), B, HW, C, 1e-10, p(out), None, need, None) == _lib.ERR_WORKSPACE
    # nothing is launched for a refused shape: the pointers are never read
    assert lib.glare_lpips_head_bf16(p(x), p(x), p(w), B, HW, 60, 1e-10, p(out), p(ws), need, None) == _lib.ERR_INVALID          # C % 8 != 0
    assert lib.glare_lpips_head_backward_bf16(p(x), p(x), p(w), B, HW, 60, 1e-10, p(out), p(x), None) == _lib.ERR_INVALID
    assert lib.glare_lpips_head_bf16(p(x), p(x), p(w), B, HW, 72, 1e-10, p(out), p(ws), need, None) == _lib.ERR_UNSUPPORTED      # no lane split
    assert lib.glare_lpips_head_bf16(None, p(x), p(w), B, HW, C, 1e-10, p(out), p(ws), need, None) == _lib.ERR_INVALID
    assert lib.glare_lpips_head_bf16(p(x), p(x), p(w), 0, HW, C, 1e-10, p(out), p(ws), need, None) == _lib.ERR_INVALID
    assert lib.glare_lpips_head_backward_bf16(p(x), p(x), p(w), B, HW, C, 1e-10, None, p(x), None) == _lib.ERR_INVALID
    assert lib.glare_lpips_head_workspace_bytes(B, HW, 60) == 0
    assert lib.glare_image_affine_f32(None, p(w), None, p(out), 1, 3, None) == _lib.ERR_INVALID
    assert lib.glare_image_affine_f32(p(out), p(w), None, p(out), 0, 3, None) == 0


@pytest.mark.parametrize("n", (1, 13, 4099))
def test_image_affine_per_element(prec, n):
    """LPIPS' scaling layer on 2 x - 1 as one fused multiply-add per element, and its backward (the product alone): one rounding each."""
    g = torch.Generator().manual_seed(n)
    x = torch.rand(n, 3, generator=g)
    x[0, 0], x[-1, 2] = 0.0, 1.0
    shift, scale = torch.tensor([-.030, -.088, -.188]).double(), torch.tensor([.458, .448, .450]).double()
    mul, add = (2.0 / scale).float(), ((-1.0 - shift) / scale).float()
    y = T.image_affine(x.cuda(), mul.cuda(), add.cuda())
    exact, tol = R.affine64(x, mul, add)
    _check_f32(y, exact, tol, "affine:%d" % n)
    # ... which is the published (2 x - 1 - shift) / scale up to the two vectors' own rounding (2 U each)
    pub = (2 * x.double() - 1 - shift) / scale
    assert float(((exact - pub).abs() / (pub.abs() + x.double().abs() * mul.double() + 1)).max()) < 4 * R.U
    gy = torch.randn(n, 3, generator=g)
    gx = T.image_affine(gy.cuda(), mul.cuda())
    exact, tol = R.affine64(gy, mul)
    _check_f32(gx, exact, tol, "affine_bwd:%d" % n)
    assert torch.equal(_bits(y), _bits(T.image_affine(x.cuda(), mul.cuda(), add.cuda())))
