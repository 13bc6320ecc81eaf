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


# ---- attention, the row softmax, the weight gradient (references of test_gpu_matrix_backward.py) ---------------------------------
@pytest.mark.parametrize("N", (1, 33, 65))
def test_attention_forward_and_backward(N):
    g = torch.Generator().manual_seed(40 + N)
    B, d = 2, 512
    q, k, v = _leaf(_rand(g, B, N, d) * 0.2), _leaf(_rand(g, B, N, d)), _leaf(_rand(g, B, N, d))
    do = _rand(g, B, N, d)
    s = q @ k.transpose(1, 2)
    out = torch.softmax(s * math.log(2.0), -1) @ v
    aq, ak, av = torch.autograd.grad((out * do).sum(), (q, k, v))
    O, L = R.attention_fp64(q.detach(), k.detach(), v.detach())
    _close(O, out.detach(), "O")
    _close(L, torch.logsumexp(s.detach() * math.log(2.0), -1) / math.log(2.0), "L")
    dq, dk, dv, D = R.attention_backward_fp64(q.detach(), k.detach(), v.detach(), O, do, L, math.log(2.0))
    if N == 1:          # one key: p = 1 whatever q and k are, both gradients vanish (dp = D up to the rounding of O)
        assert float(aq.abs().max()) == 0 and float(ak.abs().max()) == 0 and float(dq.abs().max()) < REL and float(dk.abs().max()) < REL
    else:
        _close(dq, aq, "dq")
        _close(dk, ak, "dk")
    _close(dv, av, "dv")
    _close(D, (do * out.detach()).sum(-1), "D")


def test_softmax2_rows_and_attention_ds():
    g = torch.Generator().manual_seed(44)
    n, d = 37, 24
    S, v = _leaf(_rand(g, 3, n) * 4), _rand(g, n, d)
    dO = _rand(g, 3, d)
    P = torch.softmax(S * math.log(2.0), -1)
    O = P @ v
    aS, = torch.autograd.grad((O * dO).sum(), (S,))
    P64 = R.softmax2_rows_fp64(S.detach())
    _close(P64, P.detach(), "P")
    dS, delta = R.attention_ds_fp64(P64, dO @ v.t(), dO, O.detach(), math.log(2.0))
    _close(dS, aS, "dS")
    _close(delta, (dO * O.detach()).sum(-1), "delta")


@pytest.mark.parametrize("ksize", (1, 3))
@pytest.mark.parametrize("B,H,W,Ci,Co", ((1, 1, 1, 8, 8), (1, 1, 17, 8, 16), (2, 3, 15, 16, 8), (2, 5, 7, 8, 24)))
def test_conv_weight_grad(B, H, W, Ci, Co, ksize):
    g = torch.Generator().manual_seed(H * 16 + W + ksize)
    x, gy = _rand(g, B, H, W, Ci), _rand(g, B, H, W, Co)
    dW, db = R.conv_weight_grad_fp64(x, gy, ksize)
    ref = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (Co, Ci, ksize, ksize), gy.permute(0, 3, 1, 2), padding=ksize // 2)
    _close(dW, ref, "dW")
    _close(db, gy.sum((0, 1, 2)), "db")


@pytest.mark.parametrize("fmt", sorted(R.FORMATS))
@pytest.mark.parametrize("B,N", R.EXACT_CASES)
def test_exact_attention_operands_are_exact_and_show_every_single_term(B, N, fmt):
    """The preconditions of the exact-arithmetic family: integer operands, p a power of two in [2^-6, 1], ds representable in the format's
    significand, every partial sum an exact fp32 number; and removing ANY single (i, j) term from the reference moves at least one
    output element by more than twice its bound.  (EXACT_CASE_LARGE meets all of it as well -- smallest ratio 16.0 in bf16, 127.8 in
    fp16 -- but takes half a minute per format on a CPU: test_gpu_matrix_backward.py asserts the same on the device.)"""
    m, emin = R.FORMATS[fmt]
    q, k, v, o, do, L = R.exact_attention_case(B, N)
    for t in (q, k, v, o, do, L):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= (6 if t is L else 3)
    exact, bounds, (p, ds) = R.exact_attention_bounds(q, k, v, o, do, L, m, emin)
    e = torch.log2(p)
    assert torch.equal(e, e.round()) and float(e.min()) >= -6 and float(e.max()) <= 0
    assert N == 1 or float(e.min()) < float(e.max())
    assert float((ds / p).abs().max()) < 2 ** (m + 1) and torch.equal(ds / p, (ds / p).round())          # ds = p * an integer of <= m + 1 bits
    for mag in (ds.abs() @ k.abs(), ds.abs().transpose(1, 2) @ q.abs(), p.transpose(1, 2) @ do.abs()):
        assert float(mag.max()) / float(p.min()) < 2 ** 24                                                # multiples of the smallest p: exact in fp32
    sens = R.single_term_sensitivity(q, k, do, p, ds, bounds)
    assert float(sens.min()) > 2.0, float(sens.min())
