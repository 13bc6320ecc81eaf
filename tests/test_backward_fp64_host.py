"""CPU: every fp64 restatement of tests/backward_fp64.py against fp64 AUTOGRAD of the forward operation, to 1e-12 relative
(largest |difference| over the largest |value| of the tensor).  The restatements are the references of the per-element GPU test
(test_gpu_backward_edges.py); this keeps them from being a copy of the kernels they judge."""
import math

import pytest
import torch
import torch.nn.functional as F

import backward_fp64 as R

EPS = 1e-4
REL = 1e-12


def _close(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(want.abs().max())
    assert scale > 0, what
    err = float((got - want).abs().max()) / scale
    assert err < REL, "%s: %g" % (what, err)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _leaf(t):
    return t.clone().requires_grad_(True)


def test_nll_backward():
    g = torch.Generator().manual_seed(1)
    z, mean = _leaf(_rand(g, 3, 5, 7, 3)), _leaf(_rand(g, 3, 5, 7, 3))
    g_logp = torch.tensor([0.7, 0.0, -1.3], dtype=torch.float64)
    logp = (-0.5 * ((z - mean) ** 2 + math.log(2 * math.pi))).flatten(1).sum(1)
    az, am = torch.autograd.grad((logp * g_logp).sum(), (z, mean))
    gz, gmean = R.nll_backward(z.detach(), mean.detach(), g_logp)
    _close(gz, az, "gz")
    _close(gmean, am, "gmean")


def _coupling(pre, shift, raw):
    s = torch.sigmoid(raw + 2.0) + EPS
    return (pre + shift) * s, torch.log(s)


def test_post_backward():
    g = torch.Generator().manual_seed(2)
    B, P = 3, 11
    z, h4 = _leaf(_rand(g, B, P, 3)), _leaf(_rand(g, B, P, 4) * 3)
    gout, g_logdet = _rand(g, B, P, 3), torch.tensor([0.7, 0.0, -1.3], dtype=torch.float64)
    o1, l1 = _coupling(z[..., 1], h4[..., 0], h4[..., 1])
    o2, l2 = _coupling(z[..., 2], h4[..., 2], h4[..., 3])
    out = torch.stack([z[..., 0], o1, o2], -1)
    logdet = (l1 + l2).sum(1)
    az, ah = torch.autograd.grad((out * gout).sum() + (logdet * g_logdet).sum(), (z, h4))
    gz, gh4 = R.post_backward(gout, z.detach(), h4.detach(), g_logdet, EPS)
    _close(gz, az, "gz")
    _close(gh4, ah, "gh4")


def test_pre_backward():
    g = torch.Generator().manual_seed(3)
    B, P = 3, 13
    z, f6 = _leaf(_rand(g, B, P, 3)), _leaf(_rand(g, B, P, 6) * 3)
    M, t = _leaf(_rand(g, 3, 3)), _leaf(_rand(g, 3))
    assert float((M.detach() - M.detach().t()).abs().max()) > 0.5          # M^T is not M
    gout, g_logdet = _rand(g, B, P, 3), torch.tensor([0.7, 0.0, -1.3], dtype=torch.float64)
    y = z @ M.t() + t
    outs, logs = zip(*[_coupling(y[..., i], f6[..., 2 * i], f6[..., 2 * i + 1]) for i in range(3)])
    out = torch.stack(outs, -1)
    logdet = sum(logs).sum(1)
    az, af, aM, at = torch.autograd.grad((out * gout).sum() + (logdet * g_logdet).sum(), (z, f6, M, t))
    gz, gf6, gy = R.pre_backward(gout, z.detach(), f6.detach(), g_logdet, M.detach(), t.detach(), EPS)
    _close(gz, az, "gz")
    _close(gf6, af, "gf6")
    terms = R.pre_terms(gy, z.detach()).flatten(0, 1).sum(0)
    _close(terms[:9].view(3, 3), aM, "gM")
    _close(terms[9:], at, "gt")


@pytest.mark.parametrize("B,H,W", ((1, 1, 1), (1, 1, 9), (1, 7, 1), (2, 3, 5), (2, 5, 7)))
def test_h1_backward(B, H, W):
    g = torch.Generator().manual_seed(H * 16 + W)
    z0, wz = _leaf(_rand(g, B, H, W)), _leaf(_rand(g, 64, 9))
    gh1 = _rand(g, B, H, W, 64)
    h1 = R.h1_forward(z0, wz)
    assert torch.equal(h1.detach(), F.conv2d(z0.detach().unsqueeze(1), wz.detach().view(64, 1, 3, 3), padding=1).permute(0, 2, 3, 1))
    az, aw = torch.autograd.grad((h1 * gh1).sum(), (z0, wz))
    _close(R.h1_backward_data(gh1, wz.detach()), az, "gz0")
    _close(R.h1_filter_terms(gh1, z0.detach()).flatten(0, 2).sum(0), aw, "gwz")


@pytest.mark.parametrize("swish", (False, True))
@pytest.mark.parametrize("HW,C", ((1, 64), (7, 64), (33, 32), (5, 128)))
def test_groupnorm_backward(HW, C, swish):
    g = torch.Generator().manual_seed(HW + C)
    B, eps = 2, 1e-6
    x = _leaf(_rand(g, B, HW, C) * 1.5 + 0.3)
    gamma, beta = _leaf(_rand(g, C) * 0.3 + 1), _leaf(_rand(g, C) * 0.3)
    dy = _rand(g, B, HW, C)
    y = F.group_norm(x.permute(0, 2, 1), 32, gamma, beta, eps=eps).permute(0, 2, 1)
    y = y * torch.sigmoid(y) if swish else y
    ax, ag, ab = torch.autograd.grad((y * dy).sum(), (x, gamma, beta))
    xg = x.detach().view(B, HW, 32, C // 32)
    mean = xg.mean((1, 3))
    rstd = 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False) + eps)
    dx, s1, s2, _, _ = R.groupnorm_backward(x.detach(), dy, gamma.detach(), beta.detach(), mean, rstd, swish)
    _close(dx, ax, "dx")
    _close(s1.sum(0), ab, "dbeta")
    _close(s2.sum(0), ag, "dgamma")


def test_mix_backward():
    g = torch.Generator().manual_seed(5)
    for wv in (-0.6, 0.3, 5.0):
        a, b, w = _leaf(_rand(g, 4, 24)), _leaf(_rand(g, 4, 24)), torch.tensor(wv, dtype=torch.float64, requires_grad=True)
        gout = _rand(g, 4, 24)
        s = torch.sigmoid(w)
        aa, ab, aw = torch.autograd.grad(((s * a + (1 - s) * b) * gout).sum(), (a, b, w))
        ga, gb, dw = R.mix_backward(gout, a.detach(), b.detach(), w.detach())
        _close(ga, aa, "ga")
        _close(gb, ab, "gb")
        _close(dw.reshape(1), aw.reshape(1), "dw")


@pytest.mark.parametrize("whole", (False, True))
@pytest.mark.parametrize("B", (1, 3))
def test_mean_rescale_backward(B, whole):
    g = torch.Generator().manual_seed(6 + B)
    n = 13
    h = _leaf(_rand(g, B, n) + 0.2)
    xw = _leaf(torch.rand(B, n, generator=g, dtype=torch.float64) + 0.5)
    gout = _rand(g, B, n)
    r = (h.sum() / xw.sum()).expand(B) if whole else h.sum(1) / xw.sum(1)
    ah, ax = torch.autograd.grad(((h + xw * r[:, None]) * gout).sum(), (h, xw))
    gh, gxw = R.mean_rescale_backward(gout, h.detach(), xw.detach(), whole)
    _close(gh, ah, "gh")
    _close(gxw, ax, "gxw")


@pytest.mark.parametrize("act", ("relu", "sigmoid"))
def test_act_backward(act):
    g = torch.Generator().manual_seed(7)
    x = _leaf(_rand(g, 5, 64))
    gout = _rand(g, 5, 64)
    y = torch.relu(x) if act == "relu" else torch.sigmoid(x)
    ax, = torch.autograd.grad((y * gout).sum(), (x,))
    _close(R.act_backward(gout, y.detach(), act), ax, act)
