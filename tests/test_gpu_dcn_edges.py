"""GPU: the DCN forward PER ELEMENT against the fp64 restatement of tests/dcn_fp64.py (checked on the CPU against the C oracle and F.conv2d,
its exact family proven representable and every comparison shown sensitive: test_dcn_fp64_host.py), in both 16-bit formats:
  * glare_mdcn_forward_nhwc on 16-bit x: every instantiation launch_dcn_fast can reach (dcn_fp64.LEAN: the four WN = 4 launches, the two
    plain split launches WN = 4 leaves, the six single-pass launches with the 128-pixel MT = 2 one) -- the dispatch is restated
    (dcn_fp64.lean_dispatch) and asserted; GLARE_MDCN_GENERAL_KERNEL (dcn_fwd_kernel<true>); fp32 x (dcn_fwd_kernel<false>); planar
    output with 16-bit x on 5 x 5 images, B = 4, where a 64-pixel tile spans three images;
  * glare_mdcn_forward_nhwc_fused: out16, out16 + sums, out32 + sums, on the 64- and the 128-pixel tile;
  * the drop-in glare_mdcn_forward_f32: the MFMA kernel with planar output (cpg 32 / 64, Co 64 / 128 / 256, stride 2 / dilation 2, with and
    without bias) and three dcn_generic.hip geometries, entries of test_gpu_dcn.py's GENERIC_CASES (the 1x1, conv AND deformable groups, stride 2 /
    dilation 2 with four conv groups), on the sizes below and on the entry's own; its refusals, with a NaN-filled output and workspace.
Images 1x1, 1x9, 9x1 (the right / bottom corners never exist), 5x7, 8x8 (one tile), 5x13 (65 pixels); B in {1, 3}.

Layout and poison: x sits at channel 128 of records of 256 + C channels whose other channels are NaN; the offset / mask planes have a pitch
above Ho Wo with NaN behind the plane; the output has an offset and a pitch above Co (planar: a plane above Ho Wo) inside a NaN- /
0x7B7B-filled buffer with tail rows and guards.  Every launch runs twice: the same bits; nothing outside the owned region is written.

Offsets: random of scale 0.3 and 4, and in every case the fixed positions of dcn_fp64.fixed_offsets: exactly -1, inside (-1, 0), exactly
H - 1, inside (H - 1, H), exactly H, the same for w, +-1e4 and +-3e9.  The last is beyond `int`: an out-of-image sample forms no address that
is dereferenced in any kernel -- the lean kernel sends all four corners to the out-of-range descriptor offset 2^31 (`inside` is part of
top / bot), the general kernel's load8 and the generic kernel's bilinear() are predicated on `inside` -- read in dcn.hip / dcn_generic.hip.

EQUAL: the exact family, bit for bit in every form (fp32, the once-rounded 16-bit output, the tile sums, the drop-in).  BOUNDED: the random
family within dcn_fp64.slack.  The fused outputs are the plain launch's bits (rounded once); an image's sums are the same alone and in a batch.
Measured / bound on the MI355X: profiles/attention_dcn_forward.txt."""
import pytest
import torch

import dcn_fp64 as D
import helpers_fp64 as H_
from fp64_bounds import U, _bits, assert_f32
from glare_amd import _lib, ops
from glare_amd._lib import ptr, stream_handle

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD, TAIL = 64, 3
X_OFF, X_EXTRA = 128, 256
WANT = {"wn4-co128-cpg32": (1, 4, 2, False, 4), "wn4-co256-cpg32": (2, 4, 2, False, 4), "wn4-co128-cpg64": (1, 8, 2, False, 4),
        "wn4-co256-cpg64": (2, 8, 2, False, 4), "split-co64-cpg32": (1, 4, 1, False, 2), "split-co64-cpg64": (1, 8, 1, False, 2),
        "single-co64-cpg32": (1, 4, 1, True, 2), "single-mt2-co128-cpg32": (2, 4, 2, True, 2), "single-co256-cpg32": (4, 4, 1, True, 2),
        "single-co64-cpg64": (1, 8, 1, True, 2), "single-co128-cpg64": (2, 8, 1, True, 2), "single-co256-cpg64": (4, 8, 1, True, 2)}


@pytest.fixture(params=("bf16", "fp16"))
def prec(request):
    with ops.use_precision(request.param):
        yield request.param


def _sentinel(n, f32):
    return torch.full((n,), NAN, dtype=torch.float32, device="cuda") if f32 else H_.sentinel16((n,), ops.act_dtype(), "cuda")


class _Nhwc:
    """[B n + TAIL, pitch] rows in a guarded sentinel buffer; the launch owns channels [off, off + Co) of the first B n rows"""

    def __init__(self, rows, Co, f32):
        self.rows, self.Co, self.f32, self.pitch, self.off = rows, Co, f32, Co + 24, 8
        self.flat = _sentinel((rows + TAIL) * self.pitch + 2 * GUARD, f32)
        self.body = self.flat[GUARD:GUARD + (rows + TAIL) * self.pitch].view(rows + TAIL, self.pitch)

    def owned(self):
        return self.body[:self.rows, self.off:self.off + self.Co]

    def expected(self, values):
        e = _Nhwc(self.rows, self.Co, self.f32)
        e.owned().copy_(values.reshape(self.rows, self.Co))
        return e.flat


class _Planar:
    def __init__(self, B, Co, n, plane):
        self.B, self.Co, self.n, self.plane = B, Co, n, plane
        self.flat = _sentinel(B * Co * plane + 2 * GUARD, True)
        self.body = self.flat[GUARD:GUARD + B * Co * plane].view(B, Co, plane)

    def owned(self):
        return self.body[:, :, :self.n]

    def expected(self, values_nhwc):
        e = _Planar(self.B, self.Co, self.n, self.plane)
        e.owned().copy_(values_nhwc.reshape(self.B, self.n, self.Co).transpose(1, 2))
        return e.flat


class _Dev:
    """one case's operands on the device in the poisoned layout"""

    def __init__(self, o, x_dtype, single=False):
        k, s, p, d, dg, groups = o["geom"]
        self.o, self.geom = o, o["geom"]
        B, H, W, C = o["x"].shape
        self.B, self.H, self.W, self.C, self.Co = B, H, W, C, o["w"].shape[0]
        self.Ho, self.Wo = D.out_size(H, W, k, s, p, d)
        self.n = self.Ho * self.Wo
        self.xp = X_EXTRA + C
        x = torch.full((B, H, W, self.xp), NAN, dtype=x_dtype)
        x[..., X_OFF:X_OFF + C] = o["x"].to(x_dtype)
        assert torch.equal(x[..., X_OFF:X_OFF + C].double(), o["x"]), "x is not a number of its format"
        self.x = x.cuda()
        self.plane = self.n + 3
        K = k * k
        off = torch.full((B, dg * 2 * K, self.plane), NAN, dtype=torch.float32)
        off[..., :self.n] = o["offset"]
        msk = torch.full((B, dg * K, self.plane), NAN, dtype=torch.float32)
        msk[..., :self.n] = o["mask"]
        self.off, self.msk = off.cuda(), msk.cuda()
        self.pd = ops.PackedDcn(o["w"].float().cuda(), o["bias"].float().cuda(), dg, single=single)
        self.single = single

    def nhwc(self, out, flags=0, planar=None):
        k, s, p, d, dg, groups = self.geom
        lib = _lib.lib()
        return lib.glare_mdcn_forward_nhwc(ptr(self.x), int(self.x.dtype != torch.float32), self.xp, X_OFF, ptr(self.off), self.plane,
                                           self.off.shape[1] * self.plane, ptr(self.msk), self.plane, self.msk.shape[1] * self.plane,
                                           int(self.o["is_logit"]), ptr(self.pd.packed), ptr(self.pd.bias),
                                           ptr(planar.body if planar is not None else out.body), int(planar is not None),
                                           0 if planar is not None else out.pitch, 0 if planar is not None else out.off,
                                           planar.plane if planar is not None else 0, self.B, self.C, self.H, self.W, self.Co, k, k, s, s, p, p, d, d,
                                           groups, dg, flags | (ops.MDCN_SINGLE_PASS if self.single else 0), stream_handle())

    def fused(self, out32, out16, sums, B=None, first=0):
        """images [first, first + B) of the batch"""
        k, s, p, d, dg, groups = self.geom
        B = self.B if B is None else B
        x, off, msk = self.x[first:], self.off[first:], self.msk[first:]
        o = out16 if out16 is not None else out32
        return _lib.lib().glare_mdcn_forward_nhwc_fused(ptr(x), self.xp, X_OFF, ptr(off), self.plane, self.off.shape[1] * self.plane, ptr(msk),
                                                        self.plane, self.msk.shape[1] * self.plane, int(self.o["is_logit"]), ptr(self.pd.packed),
                                                        ptr(self.pd.bias), ptr(None if out32 is None else out32.body),
                                                        ptr(None if out16 is None else out16.body), o.pitch, o.off, ptr(sums), B, self.C, self.H,
                                                        self.W, self.Co, k, k, s, s, p, p, d, d, groups, dg,
                                                        ops.MDCN_SINGLE_PASS if self.single else 0, stream_handle())


def _twice(launch):
    a, b = launch(), launch()
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y)), "two runs of one launch differ"
    return a


def _operands(c, Hh, W, B, fam, scale, dt, x_dtype, **kw):
    o = D.operands(c["C"], c["Co"], c["dg"], Hh, W, B, fam, narrow=c.get("single", False), scale=scale, **kw)
    if fam == "random":
        o["x"] = o["x"].to(x_dtype).double()
        o["w"], o["bias"] = o["w"].float().double(), o["bias"].float().double()
    return o


def _ref(o):
    dev = {n: (v.cuda() if torch.is_tensor(v) else v) for n, v in o.items()}
    return D.reference(dev)[:2]


FAMILIES = (("exact", None), ("random", 0.3), ("random", 4.0))


# ---- the lean kernel: every instantiation, plain and fused ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", D.LEAN, ids=[c["name"] for c in D.LEAN])
def test_lean_kernel_per_element(prec, c):
    dt = ops.act_dtype()
    assert D.lean_dispatch(c["C"], c["Co"], c["dg"], c["single"]) == ("fast",) + WANT[c["name"]]
    tile = D.tile_pixels(c["C"], c["Co"], c["dg"], c["single"])
    assert tile == _lib.lib().glare_mdcn_tile_pixels(c["C"], c["Co"], c["dg"], ops.MDCN_SINGLE_PASS if c["single"] else 0) == (128 if "mt2" in c["name"] else 64)
    nt, _, mt, _, wn = WANT[c["name"]]
    form = "single" if c["single"] else "split"
    for (Hh, W) in D.SIZES:
        for B in D.BS:
            for fam, scale in FAMILIES:
                o = _operands(c, Hh, W, B, fam, scale, dt, dt)
                dev = _Dev(o, dt, c["single"])
                exact, mag = _ref(o)
                tag = "%s:%dx%dx%d:%s%s" % (c["name"], B, Hh, W, fam, scale or "")
                rows = B * dev.n

                def plain():
                    out = _Nhwc(rows, c["Co"], True)
                    assert dev.nhwc(out) == 0
                    return (out.flat,)
                (flat,) = _twice(plain)
                got = flat[GUARD:-GUARD].view(rows + TAIL, -1)[:rows, 8:8 + c["Co"]].contiguous().view(B, dev.Ho, dev.Wo, c["Co"])
                keep = _Nhwc(rows, c["Co"], True)
                H_.assert_same_bits(flat, keep.expected(got), tag + " outside the owned region")
                if fam == "exact":
                    H_.assert_same_bits(got, exact.float(), tag + " EQUAL")
                else:
                    assert_f32(got, exact, D.slack(o, mag, form, dt), tag)

                # the fused form: the plain launch's bits, rounded once; sums of the fp32 values, tiles cut per image
                nt_img = -(-dev.n // tile)

                def fused(out16, want_sums, B_=B, first=0):
                    def run():
                        o16 = _Nhwc(B_ * dev.n, c["Co"], False) if out16 else None
                        o32 = None if out16 else _Nhwc(B_ * dev.n, c["Co"], True)
                        sums = torch.full((B_ * nt_img + 2,), NAN, dtype=torch.float32, device="cuda") if want_sums else None
                        assert dev.fused(o32, o16, sums, B_, first) == 0
                        return ((o16 or o32).flat,) + ((sums,) if want_sums else ())
                    return _twice(run)
                (f16,) = fused(True, False)
                H_.assert_same_bits(f16, _Nhwc(rows, c["Co"], False).expected(got.to(dt)), tag + " fused out16")
                f16s, s16 = fused(True, True)
                f32s, s32 = fused(False, True)
                H_.assert_same_bits(f16s, f16, tag + " fused out16 + sums")
                H_.assert_same_bits(f32s, flat, tag + " fused out32 + sums")
                H_.assert_same_bits(s16, s32, tag + " sums differ with the output form")
                assert bool(torch.isnan(s32[B * nt_img:]).all())
                sums = s32[:B * nt_img].view(B, nt_img)
                if fam == "exact":
                    H_.assert_same_bits(sums, D.tile_sums(exact, tile)[0].float(), tag + " EQUAL sums")
                else:
                    want, mags = D.tile_sums(got.double(), tile)
                    assert_f32(sums, want, (16 * mt * nt + 10) * U * mags + 1e-30, tag + ":sums")
                if B > 1:          # the last image alone: the same sums
                    _, alone = fused(True, True, 1, B - 1)
                    H_.assert_same_bits(alone[:nt_img], s32[(B - 1) * nt_img:B * nt_img].contiguous(), tag + " sums alone / in a batch")


# ---- dcn_fwd_kernel: GLARE_MDCN_GENERAL_KERNEL on 16-bit x, and fp32 x ---------------------------------------------------------------------
@pytest.mark.parametrize("c", D.GENERAL, ids=("co128-cpg32", "co64-cpg64", "co256-cpg64"))
@pytest.mark.parametrize("x32", (False, True), ids=("x16-general-flag", "x32"))
def test_general_kernel_per_element(prec, c, x32):
    dt = ops.act_dtype()
    assert D.general_dispatch(c["C"], c["Co"], c["dg"]) == c["want"]
    xdt = torch.float32 if x32 else dt
    for (Hh, W), B in zip(D.SIZES, (3, 1, 3, 1, 3, 3)):
        for fam, scale in FAMILIES:
            o = _operands(c, Hh, W, B, fam, scale, dt, xdt)
            dev = _Dev(o, xdt)
            exact, mag = _ref(o)
            tag = "general:%s:C%d-Co%d:%dx%dx%d:%s%s" % ("x32" if x32 else "x16", c["C"], c["Co"], B, Hh, W, fam, scale or "")
            rows = B * dev.n

            def run():
                out = _Nhwc(rows, c["Co"], True)
                assert dev.nhwc(out, 0 if x32 else ops.MDCN_GENERAL_KERNEL) == 0
                return (out.flat,)
            (flat,) = _twice(run)
            got = flat[GUARD:-GUARD].view(rows + TAIL, -1)[:rows, 8:8 + c["Co"]].contiguous().view(B, dev.Ho, dev.Wo, c["Co"])
            H_.assert_same_bits(flat, _Nhwc(rows, c["Co"], True).expected(got), tag + " outside the owned region")
            if fam == "exact":
                H_.assert_same_bits(got, exact.float(), tag + " EQUAL")
            else:
                assert_f32(got, exact, D.slack(o, mag, "split"), tag)


# ---- planar output with 16-bit x: a tile walks across several images -----------------------------------------------------------------------------
@pytest.mark.parametrize("c", (D.LEAN[2], D.LEAN[4], D.LEAN[7]), ids=lambda c: c["name"])
def test_planar_output_across_images(prec, c):
    dt = ops.act_dtype()
    for flags in (0, ops.MDCN_GENERAL_KERNEL):
        if flags and c["single"]:
            continue
        for fam, scale in FAMILIES:
            assert D.PLANAR == (5, 5, 4)
            o = _operands(c, 5, 5, 4, fam, scale, dt, dt)
            dev = _Dev(o, dt, c["single"])
            exact, mag = _ref(o)
            tag = "planar:%s:flags%d:%s%s" % (c["name"], flags, fam, scale or "")

            def run():
                out = _Planar(4, c["Co"], 25, 32)
                assert dev.nhwc(None, flags, planar=out) == 0
                return (out.flat,)
            (flat,) = _twice(run)
            got = flat[GUARD:-GUARD].view(4, c["Co"], 32)[:, :, :25].transpose(1, 2).contiguous().view(4, 5, 5, c["Co"])
            H_.assert_same_bits(flat, _Planar(4, c["Co"], 25, 32).expected(got), tag + " outside the owned region")
            if fam == "exact":
                H_.assert_same_bits(got, exact.float(), tag + " EQUAL")
            else:
                assert_f32(got, exact, D.slack(o, mag, "single" if c["single"] else "split", dt), tag)


# ---- the drop-in: NCHW fp32 everywhere ---------------------------------------------------------------------------------------------------------
DROP_IN = D.DROP_IN          # three MFMA geometries and three entries of test_gpu_dcn.py's GENERIC_CASES (on their own image size too)


@pytest.mark.parametrize("c", DROP_IN, ids=[c["name"] for c in DROP_IN])
def test_drop_in_per_element(c):
    lib = _lib.main_lib()
    groups = c.get("groups", 1)
    mfma = D.dcn_check(c["C"], c["Co"], c["dg"], groups)
    assert mfma == (not c["name"].startswith("generic"))
    if not mfma:
        from test_gpu_dcn import GENERIC_CASES
        assert tuple(D.GENERIC[[g["name"] for g in DROP_IN].index(c["name"]) - 3]) in [tuple(g) for g in GENERIC_CASES]
    for (Hh, W), B in list(zip(D.SIZES, (3, 1, 3, 1, 3, 3))) + ([(c["own"][:2], c["own"][2])] if "own" in c else []):
        Ho, Wo = D.out_size(Hh, W, c["k"], c["s"], c["p"], c["d"])
        if Ho < 1 or Wo < 1:
            continue
        for fam, scale in FAMILIES:
            o = D.operands(c["C"], c["Co"], c["dg"], Hh, W, B, fam, k=c["k"], s=c["s"], p=c["p"], d=c["d"], groups=groups, scale=scale)
            o["is_logit"] = False          # the drop-in takes mask VALUES
            if fam == "random":
                o["x"], o["w"], o["bias"], o["mask"] = o["x"].float().double(), o["w"].float().double(), o["bias"].float().double(), torch.sigmoid(o["mask"])
            if not c["bias"]:
                o["bias"] = None
            exact, mag = _ref(o)
            n = Ho * Wo
            x = o["x"].permute(0, 3, 1, 2).float().contiguous().cuda()
            off, msk, w = o["offset"].cuda(), o["mask"].float().cuda(), o["w"].float().cuda()
            bias = None if o["bias"] is None else o["bias"].float().cuda()
            ws = ops._workspace(lib.glare_mdcn_workspace_bytes(B, c["C"], Hh, W, c["Co"], c["k"], c["k"]), "cuda")
            tag = "drop-in:%s:%dx%dx%d:%s%s" % (c["name"], B, Hh, W, fam, scale or "")

            def run():
                out = _Planar(B, c["Co"], n, n)
                assert lib.glare_mdcn_forward_f32(ptr(x), ptr(off), ptr(msk), ptr(w), ptr(bias), ptr(out.body), B, c["C"], Hh, W, c["Co"], c["k"], c["k"],
                                                  c["s"], c["s"], c["p"], c["p"], c["d"], c["d"], groups, c["dg"], ptr(ws), ws.numel(), stream_handle()) == 0
                return (out.flat,)
            (flat,) = _twice(run)
            got = flat[GUARD:-GUARD].view(B, c["Co"], n).transpose(1, 2).contiguous().view(B, Ho, Wo, c["Co"])
            assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[-GUARD:]).all())
            if fam == "exact":
                H_.assert_same_bits(got, exact.float(), tag + " EQUAL")
            else:
                assert_f32(got, exact, D.slack(o, mag, "split" if mfma else "generic", bias=c["bias"]), tag)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_drop_in_refusals_leave_output_and_workspace_alone():
    """glare_mdcn_forward_f32 on a shape the MFMA kernels take (C = 64, Co = 64, dg = 2): a null operand, and a workspace that is missing or one
    byte short -- refused before the layout copy or the filter pack write anything -- and the general kernel's own two refusals (a kernel whose
    one-channel sample pass exceeds the LDS; no output pixels).  Every return stands in front of the first launch (dcn.hip, dcn_generic.hip)."""
    lib = _lib.main_lib()
    B, C, Hh, W, Co, dg = 2, 64, 5, 7, 64, 2
    assert D.dcn_check(C, Co, dg)
    x = torch.zeros(B, C, Hh, W, device="cuda")
    off, msk = torch.zeros(B, dg * 18, Hh, W, device="cuda"), torch.ones(B, dg * 9, Hh, W, device="cuda")
    w = torch.zeros(Co, C, 3, 3, device="cuda")
    need = lib.glare_mdcn_workspace_bytes(B, C, Hh, W, Co, 3, 3)
    assert need == (B * C * Hh * W + Co * C * 9) * 4 + 256 and lib.glare_mdcn_workspace_bytes(0, C, Hh, W, Co, 3, 3) == 0
    out = torch.full((B * Co * Hh * W + 2 * GUARD,), NAN, device="cuda")
    ws = torch.full((need // 4 + 64,), NAN, device="cuda")
    I, Un, Wk = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE

    def call(**ch):
        a = dict(x=ptr(x), off=ptr(off), msk=ptr(msk), w=ptr(w), out=ptr(out[GUARD:]), B=B, C=C, k=3, p=1, dg=dg, ws=ptr(ws), nws=need)
        a.update(ch)
        return lib.glare_mdcn_forward_f32(a["x"], a["off"], a["msk"], a["w"], None, a["out"], a["B"], a["C"], Hh, W, Co, a["k"], a["k"], 1, 1, a["p"], a["p"], 1, 1,
                                          1, a["dg"], a["ws"], a["nws"], stream_handle())
    for want, ch in [(I, dict(x=None)), (I, dict(off=None)), (I, dict(msk=None)), (I, dict(w=None)), (I, dict(out=None)), (I, dict(B=0)), (I, dict(dg=3)),
                     (Wk, dict(ws=None)), (Wk, dict(nws=need - 1)), (Wk, dict(nws=0)),
                     (Un, dict(C=6, dg=1, k=14, p=0)),          # general kernel: 196 taps x 64 pixels x 4 B exceed one LDS pass
                     (I, dict(C=6, dg=1, k=9, p=0))]:           # general kernel: a 9 x 9 filter on 5 x 7 leaves no output pixel
        assert call(**ch) == want, (ch, want)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all()), "a refused drop-in call wrote its output or its workspace"


def test_refusals_leave_the_output_alone(prec):
    dt = ops.act_dtype()
    lib = _lib.lib()
    c = D.LEAN[4]
    o = _operands(c, 5, 7, 2, "exact", None, dt, dt)
    dev = _Dev(o, dt)
    out = _Nhwc(2 * 35, 64, True)
    out16 = _Nhwc(2 * 35, 64, False)
    sums = torch.full((4,), NAN, dtype=torch.float32, device="cuda")
    I, Un = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED

    def call(**ch):
        a = dict(x=ptr(dev.x), x16=1, xp=dev.xp, xo=X_OFF, off=ptr(dev.off), msk=ptr(dev.msk), w=ptr(dev.pd.packed), out=ptr(out.body), planar=0, op=out.pitch,
                 oo=out.off, B=2, C=32, H=5, W=7, Co=64, kh=3, kw=3, sh=1, ph=1, dh=1, groups=1, dg=1, flags=0)
        a.update(ch)
        return lib.glare_mdcn_forward_nhwc(a["x"], a["x16"], a["xp"], a["xo"], a["off"], dev.plane, 0, a["msk"], dev.plane, 0, 0, a["w"], ptr(dev.pd.bias),
                                           a["out"], a["planar"], a["op"], a["oo"], 0, a["B"], a["C"], a["H"], a["W"], a["Co"], a["kh"], a["kw"], a["sh"], a["sh"],
                                           a["ph"], a["ph"], a["dh"], a["dh"], a["groups"], a["dg"], a["flags"], stream_handle())
    cases = [(I, dict(x=None)), (I, dict(off=None)), (I, dict(msk=None)), (I, dict(w=None)), (I, dict(out=None)), (I, dict(flags=4)), (I, dict(flags=3)),
             (I, dict(B=0)), (I, dict(sh=0)), (I, dict(dh=0)), (I, dict(dg=0)), (I, dict(groups=0)), (I, dict(C=32, dg=3)), (Un, dict(groups=2)),
             (Un, dict(C=48)), (Un, dict(Co=96)), (Un, dict(Co=320)), (Un, dict(xp=dev.xp + 4)), (Un, dict(xo=X_OFF + 4)), (Un, dict(xo=dev.xp - 24)),
             (I, dict(kh=9, kw=9, ph=0)),                       # Ho <= 0
             (I, dict(oo=out.pitch - 63)),                      # out_off + Co > out_pitch
             (Un, dict(Co=192, op=256)),                              # dcn_check admits it, no launcher has an instantiation for three 64-channel tiles
             (Un, dict(Co=192, op=256, flags=ops.MDCN_GENERAL_KERNEL)),
             (Un, dict(flags=ops.MDCN_SINGLE_PASS, kh=2, kw=2, ph=0)),          # the single-pass form exists on the lean path only (3 | kh kw)
             (Un, dict(flags=ops.MDCN_SINGLE_PASS, x16=0))]
    for want, ch in cases:
        assert call(**ch) == want, (ch, want)

    def fused(o32, o16, s, **ch):
        a = dict(flags=0, op=out.pitch, oo=out.off, kh=3, ph=1)
        a.update(ch)
        return lib.glare_mdcn_forward_nhwc_fused(ptr(dev.x), dev.xp, X_OFF, ptr(dev.off), dev.plane, 0, ptr(dev.msk), dev.plane, 0, 0, ptr(dev.pd.packed),
                                                 ptr(dev.pd.bias), o32, o16, a["op"], a["oo"], s, 2, 32, 5, 7, 64, a["kh"], a["kh"], 1, 1, a["ph"], a["ph"], 1, 1, 1, 1,
                                                 a["flags"], stream_handle())
    assert fused(None, None, ptr(sums)) == I                   # sums alone: some output must be named
    assert fused(ptr(out.body), None, None) == I               # out32 alone is the plain call
    assert fused(None, None, None) == I
    assert fused(None, ptr(out16.body), None, flags=ops.MDCN_GENERAL_KERNEL) == I
    assert fused(None, ptr(out16.body), None, op=out.pitch + 1) == I and fused(None, ptr(out16.body), None, oo=out.off + 1) == I
    assert fused(None, ptr(out16.body), ptr(sums), kh=2, ph=0) == Un          # off the lean path
    wp = torch.empty(16, dtype=torch.float32, device="cuda")
    for fn in (lib.glare_mdcn_pack_weight_f32, lib.glare_mdcn_pack_weight_single_f32):
        for a in ((None, ptr(wp), 64, 32, 3, 3, 1), (ptr(wp), None, 64, 32, 3, 3, 1), (ptr(wp), ptr(wp), 0, 32, 3, 3, 1), (ptr(wp), ptr(wp), 64, 0, 3, 3, 1),
                  (ptr(wp), ptr(wp), 64, 32, 0, 3, 1), (ptr(wp), ptr(wp), 64, 32, 3, 3, 0), (ptr(wp), ptr(wp), 64, 32, 3, 3, 3)):
            assert fn(*a, stream_handle()) == I
    assert lib.glare_mdcn_pack_weight_single_f32(ptr(wp), ptr(wp), 64, 36, 3, 3, 3, stream_handle()) == I          # 12 channels per group: not whole 8-channel chunks
    for a, want in (((0, 64, 1, 0), I), ((32, 0, 1, 0), I), ((32, 64, 0, 0), I), ((32, 64, 3, 0), I), ((128, 128, 4, ops.MDCN_SINGLE_PASS), 128), ((128, 128, 4, 0), 64),
                    ((128, 128, 2, ops.MDCN_SINGLE_PASS), 64)):
        assert lib.glare_mdcn_tile_pixels(*a) == want
    torch.cuda.synchronize()
    for t in (out, out16):
        H_.assert_same_bits(t.flat, _sentinel(t.flat.numel(), t.f32), "a refused launch wrote its output")
    assert bool(torch.isnan(sums).all())
