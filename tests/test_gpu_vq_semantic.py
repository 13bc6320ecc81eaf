"""GPU: the fused semantic guidance kernel (csrc/vq_semantic.hip: glare_vq_semantic_bf16 / _f16, glare_vq_semantic_scale_f32) through the C
ABI of both libraries, every buffer between guard bytes, per element against the fp64 restatement tests/semantic_fp64.py, and
autograd.vq_semantic against fp64 torch autograd.  Every test here fails on the parent commit: the entries do not exist.

Inputs (semantic_fp64.grid_case): q, W, b are multiples of 2^-6 in [-2, 2], so every pre-activation is a multiple of 2^-12 below 16 --
exact in fp32 in any order -- and the ReLU mask cannot depend on rounding; exact zeros occur by themselves (channel 5 has W = 0, b = 0,
token 0 has q = 0), channel 9 (b = -8) is dead everywhere.  feat is random, rounded to the 16-bit format of the precision.
Bounds (semantic_fp64.bounds, pre_roundings=0): (fp32 roundings on the element's path, counted beside the kernel's source lines) * 2^-24 *
(sum of the magnitudes of its terms), through fp64_bounds.assert_f32; where the bound is exactly 0 (nothing but zeros is added) the result
must be +-0.  Measured on the MI355X, largest err / bound over the shapes, bf16 | fp16:
    loss 0.019 | 0.005    dq 0.182 | 0.202    dW 0.108 | 0.085    db 0.052 | 0.055    (worst-case chains: sums of mixed signs stay far below)
Shapes: one token; the 64-token workgroup tile one below, at, one above (65: two workgroups of 33 and 32, waves with 9 and 8 tokens, the
unrolled round of 8 with a remainder); 257 (ragged last workgroup); 5003 (79 workgroups: the second-level sum); 32769 = 512 * 64 + 1, where
the workgroup count is capped and a workgroup's run becomes 65 tokens."""
import numpy as np
import pytest
import torch

import semantic_fp64 as S
from fp64_bounds import U, assert_f32
from glare_amd import _lib
from glare_amd._lib import stream_handle
from test_gpu_vq_ema import DEV, Guarded

pytestmark = pytest.mark.gpu

DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
SHAPES = [1, 63, 64, 65, 257, 5003, 512 * 64 + 1]
NAMES = ("loss", "dq", "dW", "db")


def _np16(feat):
    return feat.view(torch.int16).numpy()


def _abi(prec, q, W, b, feat, cout=256, n=None, short=0):
    """One call on fresh guarded copies -> (status, loss [1], dq, dW, db as numpy).  Guards are checked, inputs must be left as they were."""
    n = q.shape[0] if n is None else n
    with _lib.use_precision(prec):
        lib = _lib.lib()
        gq, gw, gb, gf = Guarded(q.numpy()), Guarded(W.numpy()), Guarded(b.numpy()), Guarded(_np16(feat))
        outs = [Guarded(np.full(s, np.nan, np.float32)) for s in ((1,), tuple(q.shape), (256, 3), (256,))]
        nws = lib.glare_vq_semantic_workspace_bytes(q.shape[0], 256)
        assert nws == S.geometry(q.shape[0])[0] * 1028 * 4
        ws = Guarded(nbytes=nws)
        rc = lib.glare_vq_semantic_bf16(gq.ptr, gw.ptr, gb.ptr, gf.ptr, n, cout, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, ws.ptr,
                                        nws - short, stream_handle())
    torch.cuda.synchronize()
    ws.read()
    assert gq.read().tobytes() == q.numpy().tobytes() and gf.read().tobytes() == _np16(feat).tobytes()
    return (rc,) + tuple(o.read().copy() for o in outs)


def _within(got, want, bound, tag):
    """per element |got - want| <= bound through assert_f32; where bound == 0 the result is zero."""
    got, want, bound = torch.from_numpy(np.ascontiguousarray(got)), want.reshape(got.shape), bound.reshape(got.shape)
    zero = bound == 0
    assert bool((got[zero] == 0).all()) and bool((want[zero] == 0).all()), tag
    assert bool(torch.isfinite(got).all()), tag
    return assert_f32(got, want, torch.where(zero, torch.ones_like(bound), bound), tag)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("N", SHAPES)
def test_loss_and_gradients_match_the_restatement_per_element(prec, N):
    q, W, b, feat = S.grid_case(N, 100 + N, DTYPE[prec])
    rc, *got = _abi(prec, q, W, b, feat)
    assert rc == 0
    want, bound = S.semantic(q, W, b, feat), S.bounds(q, W, b, feat, pre_roundings=0)
    ratios = [_within(g, w, t, name) for name, g, w, t in zip(NAMES, got, want, bound)]
    print("[%s N %d] geometry %s err / bound:" % (prec, N, S.geometry(N)), " ".join("%s %.3f" % p for p in zip(NAMES, ratios)))
    assert not got[2][5].any() and got[3][5] == 0 and got[3][9] == 0 and not got[2][9].any()      # pre == 0: gradient 0; the dead channel
    assert float(want[0]) > 0 and float(want[3].abs().max()) > 0
    # the same bits on every run
    again = _abi(prec, q, W, b, feat)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again[1:], got))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_entry_refuses_without_launching(prec):
    q, W, b, feat = S.grid_case(70, 7, DTYPE[prec])
    for kw, status in (({"cout": 128}, _lib.ERR_UNSUPPORTED), ({"n": 0}, _lib.ERR_INVALID), ({"short": 1}, _lib.ERR_WORKSPACE)):
        rc, *outs = _abi(prec, q, W, b, feat, **kw)
        assert rc == status, kw
        assert all(np.isnan(o).all() for o in outs), kw              # nothing was written


def test_scale_multiplies_the_unit_gradients_on_the_device():
    """g = 1024 * 0.25 (an fp16 loss scale times the term's weights): each gradient is the unit gradient times g to one fp32 rounding;
    without dW / db only dq is written."""
    N = 257
    q, W, b, feat = S.grid_case(N, 5, torch.bfloat16)
    _, _, dq, dW, db = _abi("bf16", q, W, b, feat)
    g = np.float32(1024 * 0.25)
    lib = _lib.main_lib()
    for params in (True, False):
        gg, units = Guarded(np.array([g], np.float32)), [Guarded(a) for a in (dq, dW, db)]
        outs = [Guarded(np.full(a.shape, np.nan, np.float32)) for a in (dq, dW, db)]
        ptrs = [o.ptr if (params or i == 0) else None for i, o in enumerate(outs)]
        _lib.check(lib.glare_vq_semantic_scale_f32(gg.ptr, N, units[0].ptr, units[1].ptr, units[2].ptr, *ptrs, stream_handle()), "scale")
        torch.cuda.synchronize()
        for i, (o, unit) in enumerate(zip(outs, (dq, dW, db))):
            got = o.read()
            if not params and i > 0:
                assert np.isnan(got).all()
                continue
            want = torch.from_numpy(unit).double() * float(g)
            _within(got, want, U * want.abs(), "scale:" + NAMES[i + 1])
        assert all(u.read().tobytes() == a.tobytes() for u, a in zip(units, (dq, dW, db)))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_autograd_node_matches_fp64_autograd(prec):
    """A.vq_semantic at B = 2, a 5 x 7 latent, times an upstream factor: the value and the gradients of quant, weight and bias against fp64
    torch autograd of F.mse_loss(relu(conv1x1(quant)), feat) * factor; feat gets none; inside data_grad_only() only quant does.
    Bound: the unit gradient's times the factor, plus the scale launch's one rounding."""
    import torch.nn.functional as F

    from glare_amd import autograd as A
    from glare_amd import ops

    B, h, w, factor = 2, 5, 7, 3.0
    q, W, b, feat = S.grid_case(B * h * w, 11, DTYPE[prec])
    q64, W64, b64 = (t.double().requires_grad_(True) for t in (q, W, b))
    ref = F.mse_loss(F.relu(F.conv2d(q64.t().reshape(1, 3, -1, 1), W64.view(256, 3, 1, 1), b64)), feat.double().t().reshape(1, 256, -1, 1))
    (ref * factor).backward()
    unit = S.bounds(q, W, b, feat, pre_roundings=0)

    def leaves():
        return (q.view(B, h, w, 3).to(DEV).requires_grad_(True), W.view(256, 3, 1, 1).to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True),
                feat.view(B, h, w, 256).to(DEV).requires_grad_(True))

    with ops.use_precision(prec):
        qd, Wd, bd, fd = leaves()
        loss = A.vq_semantic(qd, Wd, bd, fd)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        (loss * factor).backward()
        _within(loss.detach().cpu().reshape(1).numpy(), ref.detach().reshape(1), unit[0].reshape(1), "value")
        assert fd.grad is None and qd.grad.shape == qd.shape and Wd.grad.shape == Wd.shape
        for name, got, want, tol in (("dq", qd.grad, q64.grad, unit[1]), ("dW", Wd.grad, W64.grad, unit[2]), ("db", bd.grad, b64.grad, unit[3])):
            _within(got.cpu().numpy().reshape(want.shape), want, factor * tol + U * want.abs(), name)
        qd2, Wd2, bd2, fd2 = leaves()
        with A.data_grad_only():
            (A.vq_semantic(qd2, Wd2, bd2, fd2) * factor).backward()
        assert torch.equal(qd2.grad, qd.grad) and Wd2.grad is None and bd2.grad is None and fd2.grad is None
