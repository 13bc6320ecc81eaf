"""GPU: the fused coupling step of the flow's reverse pass (csrc/flow_fused.hip, glare_flow_step_fused_bf16 behind ops.flow_fused_image and
ops.flow_step_fused) PER ELEMENT against the fp64 restatement of tests/flow_fused_fp64.py (checked on the CPU against the oracle's FlowStep, its
exact family proven representable and every comparison shown sensitive: test_flow_fused_fp64_host.py), in both 16-bit formats.

Sizes (B, H, W), flow_fused_fp64.SIZES: (3,1,1) every halo pixel outside the image; (2,1,41), (2,17,1) a one-pixel axis, the second tile a single
column / row; (1,16,40) exactly one tile, block 23's padding lanes live; (2,17,41) 2 x 2 tiles, seams where the halo is another tile's pixels,
region pixels beyond the image read a clamped ftA; (3,33,81) 3 x 3 tiles, one with every halo pixel inside the image.

Layout and poison: ftA at (pitch 192, offset 64) and (68, 4), hF at (16, 8), (8, 0) and (12, 4); every float of ftA and hF outside the window read
is NaN (the two unread floats of each 8, the other steps' records), so a finite z_out within its bound proves nothing else is read.  z_out lives
inside a NaN-filled buffer with guards that must keep their bits; z_in must keep its bits; a second launch gives the same bits.

Families: the three exact variants ("int", "act_lo", "wz_lo": h4 is exact, the bound is flow_tail's few fp32 roundings, so one wrong tap, channel,
halo pixel, image or padding lane is a unit error) and the random family within the bound counted in flow_fused_fp64's header.  Two values of
eps.  Two chained steps issued as decode_nhwc issues them.  The refusals of the C ABI.  Every bound goes through tolerances.within(.., 1.0, ..)."""
import functools

import pytest
import torch

import flow_fused_fp64 as R
from fp64_bounds import _bits, _tag
from glare_amd import _lib, ops
from glare_amd._lib import host_f32, ptr, stream_handle
from tolerances import within

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64
FAR_EPS = 0.3
INVALID, UNSUPPORTED = -1, -4          # GLARE_ERR_INVALID, GLARE_ERR_UNSUPPORTED (test_capi.py pins the header's values)


@pytest.fixture(params=("bf16", "fp16"))
def prec(request):
    with ops.use_precision(request.param):
        yield request.param


@functools.lru_cache(maxsize=None)
def _case(size, family, dtype, eps):
    """operands and the fp64 reference, computed once on the CPU and left unchanged"""
    o = R.operands(*size, family, dtype, eps=eps)
    exact, bound, _ = R.step_fp64(o, dtype)
    return o, exact, bound


def _poisoned(window, pitch, off):
    """[B, H, W, c] -> a NaN-filled [B, H, W, pitch] device buffer with the window at channel `off`"""
    buf = torch.full(window.shape[:3] + (pitch,), NAN, dtype=torch.float32)
    buf[..., off:off + window.shape[3]] = window
    return buf.cuda()


def _image(o):
    return ops.flow_fused_image(*(o[n].cuda() for n in ("wz", "w2", "b2", "w4", "b4")))


class _Out:
    """z_out inside a NaN-filled buffer with a guard in front of it and behind it"""

    def __init__(self, shape):
        n = shape[0] * shape[1] * shape[2] * 3
        self.flat = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device="cuda")
        self.fill = _bits(self.flat).clone()
        self.view = self.flat[GUARD:GUARD + n].view(*shape[:3], 3)

    def guards_kept(self):
        b = _bits(self.flat)
        return torch.equal(b[:GUARD], self.fill[:GUARD]) and torch.equal(b[-GUARD:], self.fill[-GUARD:])

    def untouched(self):
        return torch.equal(_bits(self.flat), self.fill)


def _check(got, exact, bound, tag):
    assert got.dtype == torch.float32 and got.shape == exact.shape
    assert bool(torch.isfinite(got).all()), tag + ": a NaN was read"
    return within(float(((got.double().cpu() - exact).abs() / bound).max()), 1.0, _tag(tag))


def _run(o, image, z_in, a_lay, f_lay):
    """one launch, twice: the same bits, the guards and z_in kept -> z_out"""
    ftA, hF = _poisoned(o["ftA"], *a_lay), _poisoned(o["hF"][..., :6], *f_lay)
    before = _bits(z_in).clone()
    outs = []
    for _ in range(2):
        out = _Out(z_in.shape)
        ops.flow_step_fused(z_in, out.view, ftA, a_lay[1], image, hF, f_lay[1], o["M"].flatten().tolist(), o["t"].tolist(), o["eps"])
        assert out.guards_kept(), "written outside z_out"
        outs.append(out.view)
    assert torch.equal(_bits(z_in), before), "z_in was written"
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two runs of one launch differ"
    return outs[0]


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("size", R.SIZES, ids=["%dx%dx%d" % s for s in R.SIZES])
def test_fused_step_per_element(prec, size, family):
    """every pitch / offset pair at eps = 1e-4; the far eps on the tightest and on the widest layout"""
    dtype = ops.act_dtype()
    for eps, layouts in ((R.FLOW_EPS, [(a, f) for a in R.A_LAYOUTS for f in R.F_LAYOUTS]), (FAR_EPS, [(R.A_LAYOUTS[1], R.F_LAYOUTS[1]), (R.A_LAYOUTS[0], R.F_LAYOUTS[0])])):
        o, exact, bound = _case(size, family, dtype, eps)
        image = _image(o)
        z_in = o["z"].cuda()
        first = None
        for a_lay, f_lay in layouts:
            got = _run(o, image, z_in, a_lay, f_lay)
            _check(got, exact, bound, "fused:%s:%dx%dx%d:eps%g:a%d+%d:f%d+%d" % ((family,) + size + (eps,) + a_lay + f_lay))
            first = got if first is None else first
            assert torch.equal(_bits(got), _bits(first)), "the result depends on the pitch or the offset"


def test_two_chained_steps_as_decode_issues_them(prec):
    """ping-pong buffers, offsets 64 s and 8 s into ONE ftA / hF record per pixel, two different filter images; the second step's bound takes the
    first step's bound as its input error (on z0 through |wz|, on z0, z1, z2 through the tail)"""
    dtype = ops.act_dtype()
    size = (2, 17, 41)
    steps = [R.random_operands(*size, seed=s) for s in (1, 2)]
    ftA = torch.cat([o["ftA"] for o in steps], -1).cuda()                                          # [B, H, W, 2 * 64]
    rec = torch.full(size + (16,), NAN, dtype=torch.float32)                                       # 6 of every 8 written and read
    for s, o in enumerate(steps):
        rec[..., 8 * s:8 * s + 6] = o["hF"][..., :6]
    hF = rec.cuda()
    images = [_image(o) for o in steps]
    z = steps[0]["z"].cuda()
    zs = [z.clone(), torch.full_like(z, NAN)]
    for s, o in enumerate(steps):
        ops.flow_step_fused(zs[s & 1], zs[(s + 1) & 1], ftA, 64 * s, images[s], hF, 8 * s, o["M"].flatten().tolist(), o["t"].tolist(), o["eps"])
        if s == 0:
            mid = zs[1].clone()
    e1, b1, _ = R.step_fp64(steps[0], dtype)
    _check(mid, e1, b1, "chained:step0")
    o2 = dict(steps[1], z=e1)
    e2, b2, _ = R.step_fp64(o2, dtype, ez=b1)
    assert bool((b2 > R.step_fp64(o2, dtype)[1]).all())          # the input error is in the bound
    _check(zs[0], e2, b2, "chained:step1")


def test_refusals_leave_z_out_alone(prec):
    o = R.random_operands(2, 3, 5)
    B, H, W = 2, 3, 5
    image = _image(o)
    z_in = o["z"].cuda()
    ftA, hF = _poisoned(o["ftA"], 192, 64), _poisoned(o["hF"][..., :6], 16, 8)
    M, t = host_f32(o["M"].flatten().tolist(), 9), host_f32(o["t"].tolist(), 3)
    out = _Out((B, H, W))
    fn = _lib.lib().glare_flow_step_fused_bf16

    def call(**kw):
        a = dict(z_in=ptr(z_in), z_out=ptr(out.view), ftA=ptr(ftA), a_pitch=192, a_off=64, image=ptr(image), hF=ptr(hF), f_pitch=16, f_off=8, B=B, H=H, W=W,
                 M=M, t=t)
        a.update(kw)
        return fn(a["z_in"], a["z_out"], a["ftA"], a["a_pitch"], a["a_off"], a["image"], a["hF"], a["f_pitch"], a["f_off"], a["B"], a["H"], a["W"], a["M"],
                  a["t"], o["eps"], stream_handle())

    bad = [(dict(z_in=None), INVALID), (dict(z_out=None), INVALID), (dict(ftA=None), INVALID), (dict(image=None), INVALID), (dict(hF=None), INVALID),
           (dict(M=None), INVALID), (dict(t=None), INVALID), (dict(z_in=ptr(out.view)), INVALID),
           (dict(B=0), INVALID), (dict(B=-1), INVALID), (dict(H=0), INVALID), (dict(H=-1), INVALID), (dict(W=0), INVALID), (dict(W=-1), INVALID),
           (dict(a_pitch=190), UNSUPPORTED), (dict(a_off=62), UNSUPPORTED), (dict(f_pitch=14), UNSUPPORTED), (dict(f_off=2), UNSUPPORTED),
           (dict(a_pitch=64, a_off=4), UNSUPPORTED), (dict(a_off=132), UNSUPPORTED), (dict(f_pitch=8, f_off=4), UNSUPPORTED), (dict(f_off=12), UNSUPPORTED),
           (dict(image=ptr(image) + 4), INVALID), (dict(ftA=ptr(ftA) + 4), INVALID), (dict(hF=ptr(hF) + 8), INVALID)]
    for kw, want in bad:
        assert call(**kw) == want, (kw, want)
        torch.cuda.synchronize()
        assert out.untouched(), kw
    assert call() == 0          # the same arguments without the fault: the step runs
    torch.cuda.synchronize()
    assert out.guards_kept() and bool(torch.isfinite(out.view).all())
    exact, bound, _ = R.step_fp64(o, ops.act_dtype())
    _check(out.view, exact, bound, "capi:2x3x5")
