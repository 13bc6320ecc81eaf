"""CPU: every fp64 restatement of tests/loss_fp64.py against an INDEPENDENT fp64 reference -- autograd of the torch expression the
reference model evaluates, oracle.torch_ref's SSIM / MS-SSIM run in double, torch.optim.Adam on float64 parameters, ATen's
_amp_update_scale_ -- to 1e-12 relative (largest |difference| over the largest |value| of the tensor), and against the values and
the gradient the reference produced in fp32 (tests/golden/msssim.npz).  The restatements are the references of the per-element
GPU test (test_gpu_loss_update_edges.py); this keeps them from being a copy of the kernels they judge.  The CONDITIONS that test
relies on in its inputs (ties in the max-pool windows, the planted specials of the pixel losses, flat SSIM windows) are asserted
here, on the same builders."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_fp64 as R
from oracle import torch_ref as O

REL = 1e-12
GRAD_REL = 1e-10          # SSIM gradients: fp64's own rounding of E[xx] - mu^2 is amplified by 1 / C2 = 1.1e3, twice in d / d E[xx]
C1, C2 = 0.01 ** 2, 0.03 ** 2          # value range 1


def _close(got, want, what, rel=REL):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(want.abs().max())
    assert scale > 0, what
    err = float((got - want).abs().max()) / scale
    assert err < rel, "%s: %g" % (what, err)


def _leaf(t):
    return t.clone().requires_grad_(True)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ---- clamp, pixel losses, sigmoid ------------------------------------------------------------------------------------------------
def _model_l1(rec, real_H):
    """VQLLFLOWD_model.py:213-217, rec and real_H NCHW"""
    sr = rec.clamp(0, 1)
    not_nan_mask = ~torch.isnan(sr)
    sr = torch.where(torch.isnan(sr), torch.zeros_like(sr), sr)          # sr[isnan(sr)] = 0, out of place
    return sr, ((sr - real_H) * not_nan_mask).abs().mean()


def test_clamp01_and_backward():
    x = R.clamp_inputs(257, 1).double()
    assert torch.isnan(x).sum() == 2 and len(R.CLAMP_SPECIALS) == 12
    xl = _leaf(x)
    sr, _ = _model_l1(xl, torch.zeros_like(x))
    g = torch.randn(257, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    (ag,) = torch.autograd.grad((sr * g).sum(), xl)
    assert torch.equal(R.clamp01(x), sr.detach())
    assert torch.equal(R.clamp01_backward(x, g), ag)
    # the closed interval passes, one ulp outside does not, NaN does not
    spec = dict(zip(R.CLAMP_SPECIALS[:10], R.clamp01_pass(x[:10]).tolist()))
    assert spec[0.0] and spec[1.0] and spec[R.F32_TINY] and not spec[1.0 + 2.0 ** -23] and not spec[-3 * R.F32_TINY]
    assert not R.clamp01_pass(x[10:12]).any()


@pytest.mark.parametrize("shape", R.L1_SHAPES[:4])
def test_l1_losses(shape):
    rec32, gt32 = R.l1_inputs(shape, 11)
    variants = [(rec32, gt32)]
    if rec32.numel() == 1:          # one element: each special on its own
        variants = []
        for name in R.L1_SPECIALS:
            r = rec32.clone()
            R.l1_plant(r, gt32, 0, 0, name)
            variants.append((r, gt32))
    n = rec32.numel()
    for r32, g32 in variants:
        rec, gt = r32.double(), g32.double()
        rl = _leaf(_nchw(rec))
        _, loss = _model_l1(rl, gt)
        (ag,) = torch.autograd.grad(loss, rl)
        loss = loss.detach()
        terms, rloss, sign = R.l1_clamp(rec, gt)
        assert abs(float(rloss - loss)) <= REL * float(loss) and terms.shape == rec.shape
        assert torch.equal(sign / n, _nhwc(ag))
        # the plain form on a draw without NaN / inf, then with them
        clean = torch.where(torch.isfinite(rec), rec, torch.full_like(rec, 0.5))
        cl = _leaf(_nchw(clean))
        loss = (cl - gt).abs().mean()
        (ag,) = torch.autograd.grad(loss, cl)
        loss = loss.detach()
        _, rloss, sign = R.l1_plain(clean, gt)
        assert abs(float(rloss - loss)) <= REL * float(loss)
        assert torch.equal(sign / n, _nhwc(ag))
        _, rloss, sign = R.l1_plain(rec, gt)
        want = (_nchw(rec) - gt).abs().mean()
        assert torch.equal(rloss.isnan(), want.isnan()) and (rloss.isnan() or rloss == want)
        assert torch.equal(torch.isnan(sign), torch.isnan(rec))


@pytest.mark.parametrize("shape", R.L1_SHAPES)
def test_l1_inputs_hold_every_special_in_every_sample(shape):
    rec, gt = R.l1_inputs(shape, 11)
    if rec.numel() == 1:
        for name in R.L1_SPECIALS:
            r = rec.clone()
            R.l1_plant(r, gt, 0, 0, name)
            assert R.l1_has(r, gt, 0, name), name
        return
    for b in range(shape[0]):
        for name in R.L1_SPECIALS:
            assert R.l1_has(rec, gt, b, name), (b, name)
    inside = (rec >= 0) & (rec <= 1)
    assert 0.5 < float(inside.float().mean()) < 0.95          # both sides of the clamp are populated


def test_sigmoid():
    x = torch.tensor([0.0, 88.0, -88.0, 104.0, -104.0, 3.0, -0.3], dtype=torch.float64)
    _close(R.sigmoid(x), 1.0 / (1.0 + torch.exp(-x)), "sigmoid")


# ---- pools and MSE ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((1, 2, 2, 1), (1, 3, 2, 3), (2, 5, 7, 3), (1, 8, 10, 3)))
def test_avgpool2(shape):
    x = torch.rand(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    _close(R.avgpool2(x), _nhwc(F.avg_pool2d(_nchw(x), (2, 2))), "avgpool2")


@pytest.mark.parametrize("big", (65504.0, 3.3895313892515355e38))
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES)
def test_maxpool2_and_backward(shape, big):
    x = R.maxpool_inputs(shape, big, 5).double()
    B, H, W, C = shape
    xl = _leaf(_nchw(x))
    y = F.max_pool2d(xl, 2, 2)
    g = torch.randn(B, H // 2, W // 2, C, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    (ag,) = torch.autograd.grad(y, xl, _nchw(g))
    assert torch.equal(R.maxpool2(x), _nhwc(y.detach()))
    assert torch.equal(R.maxpool2_backward(x, g), _nhwc(ag))


def test_maxpool_inputs_tie():
    """at least half of all windows of every shape hold a tie for the maximum; over the shapes, each of the four positions is the
    first maximum of some window and each of the six position pairs ties for the maximum somewhere"""
    firsts, pairs = set(), set()
    for big in (65504.0, 3.3895313892515355e38):
        for shape in R.MAXPOOL_SHAPES:
            x = R.maxpool_inputs(shape, big, 5).double()
            w = R._windows(x)
            is_max = (w == w.amax(-1, keepdim=True)).reshape(-1, 4)
            assert float((is_max.sum(-1) >= 2).double().mean()) >= 0.5, shape
            firsts |= set(R.maxpool2_first(x).reshape(-1, 4).double().argmax(-1).tolist())
            for a, b in R.PAIRS:
                if bool((is_max[:, a] & is_max[:, b]).any()):
                    pairs.add((a, b))
            assert bool((x == big).any()) or x.numel() < 16
        assert firsts == {0, 1, 2, 3} and pairs == set(R.PAIRS)


def test_mse():
    g = torch.Generator().manual_seed(7)
    a, b = _leaf(torch.randn(4099, dtype=torch.float64, generator=g)), torch.randn(4099, dtype=torch.float64, generator=g)
    loss = F.mse_loss(a, b)
    (ag,) = torch.autograd.grad(loss * -3.5, a)
    loss = loss.detach()
    assert abs(float(R.mse(a.detach(), b) - loss)) < REL * float(loss)
    _close(R.mse_backward(a.detach(), b, -3.5), ag, "mse_backward")


# ---- SSIM ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def oracle64(monkeypatch):
    """oracle.torch_ref's ssim / msssim with the window kept in double: the outer product of the float32 1-D window, exact"""
    def create_window(window_size, channel=1):
        w2 = R.window2d(R.gaussian_window(window_size))
        return w2[None, None].expand(channel, 1, window_size, window_size).contiguous()
    monkeypatch.setattr(O, "_create_window", create_window)
    return O


@pytest.mark.parametrize("shape", ((2, 12, 17, 3, 11), (1, 11, 11, 3, 11), (1, 5, 7, 3, 5), (1, 3, 3, 1, 3), (1, 1, 4, 2, 1), (1, 23, 25, 3, 11)))
@pytest.mark.parametrize("family", ("random", "bright1e-2"))
def test_ssim_one_level(oracle64, shape, family):
    B, H, W, C, ws = shape
    x32, y32 = R.ssim_inputs(shape, family, 13)
    x, y = x32.double(), y32.double()
    w1 = R.gaussian_window(ws)
    assert ws == min(11, H, W)
    xl = _leaf(_nchw(x))
    sim, cs = oracle64.ssim(xl, _nchw(y), window_size=11, val_range=1)
    g_sim, g_cs = 0.7, -0.4
    (ag,) = torch.autograd.grad(g_sim * sim + g_cs * cs, xl)
    mom, rs, rc = R.ssim_forward(x, y, w1, C1, C2)
    assert mom.shape == (B, H - ws + 1, W - ws + 1, C, 5)
    assert abs(float(rs - sim.detach())) < REL and abs(float(rc - cs.detach())) < REL
    gx = R.ssim_backward(x, y, R.ssim_adjoints(mom, C1, C2, g_sim, g_cs), w1)
    _close(gx, _nhwc(ag), "gx", GRAD_REL)
    # the adjoints themselves: autograd through the maps from the moments
    ml = _leaf(mom)
    cmap, smap = R.ssim_maps(ml, C1, C2)
    (am,) = torch.autograd.grad(g_sim * smap.mean() + g_cs * cmap.mean(), ml)
    _close(R.ssim_adjoints(mom, C1, C2, g_sim, g_cs), am[..., [0, 2, 4]], "adjoints", GRAD_REL)


@pytest.mark.parametrize("H,W", ((24, 26), (23, 25), (48, 40)))
def test_ssim_two_level_chain_and_msssim(oracle64, H, W):
    """two levels joined by the 2x2 average pool (g_next; odd sizes: the last row and column receive none of it), then all five"""
    x32, y32 = R.ssim_inputs((2, H, W, 3), "random", 17)
    x, y = x32.double(), y32.double()
    xl = _leaf(_nchw(x))
    s0, c0 = oracle64.ssim(xl, _nchw(y), val_range=1)
    x1, y1 = F.avg_pool2d(xl, (2, 2)), F.avg_pool2d(_nchw(y), (2, 2))
    s1, c1 = oracle64.ssim(x1, y1, val_range=1)
    g = (0.0, 0.9, 0.6, -0.5)
    (ag,) = torch.autograd.grad(g[0] * s0 + g[1] * s1 + g[2] * c0 + g[3] * c1, xl)
    w0, w1 = R.gaussian_window(min(11, H, W)), R.gaussian_window(min(11, H // 2, W // 2))
    xp, yp = R.avgpool2(x), R.avgpool2(y)
    m0, m1 = R.ssim_moments(x, y, w0), R.ssim_moments(xp, yp, w1)
    g_next = R.ssim_backward(xp, yp, R.ssim_adjoints(m1, C1, C2, g[1], g[3]), w1)
    gx = R.ssim_backward(x, y, R.ssim_adjoints(m0, C1, C2, g[0], g[2]), w0, g_next)
    _close(gx, _nhwc(ag), "gx two levels", GRAD_REL)
    if H % 2:
        plain = R.ssim_backward(x, y, R.ssim_adjoints(m0, C1, C2, g[0], g[2]), w0)
        assert torch.equal(gx[:, -1], plain[:, -1]) and torch.equal(gx[:, :, -1], plain[:, :, -1])
    if min(H, W) >= 32:
        xl = _leaf(_nchw(x))
        val = oracle64.msssim(xl, _nchw(y), val_range=1, normalize=True)
        (ag,) = torch.autograd.grad(val, xl)
        h, w, windows = H, W, []
        for _ in range(5):
            windows.append(R.gaussian_window(min(11, h, w)))
            h, w = h // 2, w // 2
        assert len(windows[-1]) < 11          # a window shorter than 11
        rv, rg = R.msssim_chain(x, y, windows, C1, C2, True)
        # MSSSIM_WEIGHTS: the oracle keeps them in float32
        assert abs(float(rv - val.detach())) < 1e-7
        _close(rg, _nhwc(ag.detach()), "msssim gx", 1e-6)


def test_msssim_against_reference_vectors():
    """the value and the gradient the reference produced in fp32 (tests/golden/msssim.npz).  Its own error: fp32 convolutions
    (2^-24 per rounding, 121 taps) through the 1 / C2 = 1.1e3 amplification of the variance cancellation, so 1e-5 on the value and 1e-4
    of the largest gradient element is what an fp32 evaluation can be held to"""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msssim.npz"))
    x, y = (_nhwc(torch.from_numpy(g[k]).double()) for k in ("sr", "gt"))
    h, w, windows = x.shape[1], x.shape[2], []
    for _ in range(5):
        windows.append(R.gaussian_window(min(11, h, w)))
        h, w = h // 2, w // 2
    val, gx = R.msssim_chain(x, y, windows, C1, C2, True)
    assert abs(float(val) - float(g["msssim_norm"])) < 1e-5
    _close(gx, _nhwc(torch.from_numpy(g["grad"]).double()), "grad", 1e-4)
    plain, _ = R.msssim_chain(x, y, windows, C1, C2, False)
    assert abs(float(plain) - float(g["msssim_plain"])) < 1e-5
    _, s0, c0 = R.ssim_forward(x, y, windows[0], C1, C2)
    assert abs(float(s0) - float(g["ssim0"])) < 1e-5 and abs(float(c0) - float(g["cs0"])) < 1e-5


@pytest.mark.parametrize("family", ("flat0", "flat1", "flat.25/.75"))
def test_flat_families_have_no_spread(family):
    for shape in R.SSIM_SHAPES[:5]:
        x, y = R.ssim_inputs(shape, family, 1)
        for img in (x, y):
            assert float(R.window_spread(img, shape[4]).abs().max()) == 0.0
    x, y = R.ssim_inputs(R.SSIM_SHAPES[1], "random", 1)
    assert float(R.window_spread(x, 11).min()) > 0.0


# ---- Adam ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas,wd", (((0.9, 0.999), 0.0), ((0.5, 0.9), 0.0), ((0.9, 0.999), 0.01), ((0.5, 0.9), 0.01)))
def test_adam_against_torch_optim(betas, wd):
    g = torch.Generator().manual_seed(19)
    n, lr, eps = 257, 1e-3, 1e-8
    p = torch.nn.Parameter(torch.randn(n, dtype=torch.float64, generator=g))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    w, m, v = p.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 8):
        grad = torch.randn(n, dtype=torch.float64, generator=g) * 10.0 ** (step - 4)
        p.grad = grad.clone()
        opt.step()
        # grad_scale / loss_scale / lr_mul: the same step on a pre-scaled gradient and a split learning rate
        w, m, v = R.adam_step(w, grad * 6.0, m, v, lr * 4, betas[0], betas[1], eps, wd, step, grad_scale=0.5, loss_scale=3.0, lr_mul=0.25)
        st = opt.state[p]
        _close(w, p.detach(), "w step %d" % step)
        _close(m, st["exp_avg"], "m step %d" % step)
        _close(v, st["exp_avg_sq"], "v step %d" % step)
    bc1, bc2s = R.adam_bias(betas[0], betas[1], 7)
    assert abs(bc1 - (1 - betas[0] ** 7)) < 1e-15 and abs(bc2s ** 2 - (1 - betas[1] ** 7)) < 1e-15


# ---- the grad scaler -------------------------------------------------------------------------------------------------------------
def test_scaler_update_against_aten_bit_for_bit():
    assert hasattr(torch, "_amp_update_scale_"), "torch._amp_update_scale_ is missing from this torch"
    kept = 0
    for row in R.SCALER_TABLE:
        scale, tracker, found, growth, backoff, interval = row
        s = torch.tensor([scale], dtype=torch.float32)
        t = torch.tensor([tracker], dtype=torch.int32)
        torch._amp_update_scale_(s, t, torch.tensor([float(found)]), growth, backoff, interval)
        rs, rt = R.scaler_update(scale, tracker, found, growth, backoff, interval)
        assert R.f32_bits(rs) == R.f32_bits(s.numpy()[0]) and rt == int(t), (row, float(rs), rt, float(s), int(t))
        assert not R.nonfinite_bits(R.f32_bits(rs)), row
        kept += found == 0 and tracker + 1 == interval and R.f32_bits(rs) == R.f32_bits(scale)
    assert kept == 2          # the two rows whose grown scale would be inf keep theirs


def test_nonfinite_predicate():
    for bits, want in ((0x7f800000, True), (0xff800000, True), (0x7fc00000, True), (0xffc00000, True), (0x7f800001, True),
                       (0x7f7fffff, False), (0xff7fffff, False), (0x00000001, False), (0x807fffff, False), (0, False), (0x80000000, False)):
        v = np.array(bits, dtype=np.uint32).view(np.float32)
        assert R.nonfinite_bits(bits) == want == (not np.isfinite(v)), hex(bits)
        assert R.f32_bits(v) == bits or bits in (0x7f800001,)          # (a signalling NaN may be quieted on the way)
