"""GPU: the forward convolutions PER ELEMENT against the fp64 restatements of tests/conv_fp64.py (checked on the CPU against F.conv2d,
F.interpolate, F.pad and fp64 autograd: test_conv_fp64_host.py), in both 16-bit formats: the implicit-GEMM kernel (conv_igemm*.hip: 3x3
stride 1 and 2, 1x1, the sub-pixel form; LDS-staged, planar fp32 and general epilogues; the HILO and GNP instantiations; grouped launches;
the data-gradient pack), the weight-stationary 1x1 kernel (conv1x1.hip: plain, hi / lo, split, one filter per image) and conv_small.hip.

Every output lives in a buffer larger than what the launch owns, filled with a sentinel first (int16 0x7B7B; NaN for fp32): the channels
outside [out_off, out_off + cout), the [OH OW, plane_pitch) tail of every plane and 64 guard elements in front of and behind the tensor
must still hold it.  Inputs and residuals are channel windows (offsets multiples of 8) of wider NaN-filled buffers: a read outside a
window poisons the result.  B >= 2 wherever the geometry allows.  Every launch runs twice and must give the same bits.

Two kinds of assertion (fp64_bounds.py; U = 2^-24):
  EQUAL    integer operands (conv_fp64.int_operands; test_conv_fp64_host.py checks that every result is representable and that one removed
           product, a shifted halo column, a row of the next image, the neighbour's bias and a dropped K tail all change the expected bits):
           every product and every partial sum of every order is exact in fp32, so an fp32 output must equal the fp64 value and a 16-bit
           output the restatement's documented roundings (conv_fp64's docstring), bit for bit -- the WHOLE buffer, sentinel included.
  BOUNDED  normal operands that are 16-bit numbers (every MFMA product exact):
           |got - exact| <= 0.5 ulp16(exact) + 2 U (Kp + 1) sum |terms| + 2 U |.| per epilogue addition
           with Kp the products the kernel multiplies, zero-filled K stages included (the rule of test_gpu_disc_kernels.py); fp32 outputs take
           the slack alone; the LDS-staged epilogue adds the half ulp16 of its rounding in front of the residual add; sigmoid / swish
           their own evaluation (test_gpu_backward_edges._sigmoid_rel with two argument roundings: __expf) on the accumulator's error;
           the fp32-class form its dropped sum |x_lo| |w_lo| and the pair's second rounding; conv_small (k k cin + 1) U sum |terms|.
Which kernel and epilogue a case takes is asserted from the dispatch restated in conv_fp64 (pick_variant, conv_pick_epilogue,
glare_conv1x1_ws_supported) and, for the weight-stationary kernel, from ops._ws_eligible and a spy on the wrapper that launches it.

Measured / bound on the MI355X: profiles/conv_forward.txt."""
import ctypes

import pytest
import torch

import conv_fp64 as C
import helpers_fp64 as H
from fp64_bounds import U, _bits, assert_f32, assert_rounded
from glare_amd import _lib, ops
from tolerances import within

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64          # sentinel elements in front of and behind every output tensor


@pytest.fixture(params=("bf16", "fp16"))
def prec(request):
    with ops.use_precision(request.param):
        yield request.param


@pytest.fixture
def ws_calls(monkeypatch):
    """every launch of the weight-stationary kernel through ops.conv2d, recorded"""
    calls = []
    real = ops._conv1x1_ws
    monkeypatch.setattr(ops, "_conv1x1_ws", lambda *a, **kw: (calls.append(a[1]), real(*a, **kw))[1])
    return calls


def test_constants_agree():
    assert (ops.OUT_NHWC_BF16, ops.OUT_NHWC_F32, ops.OUT_PLANAR_F32, ops.OUT_PLANAR_BF16) == (C.NHWC16, C.NHWC32, C.PLANAR32, C.PLANAR16)
    assert C.U == U


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
class _Out:
    """an output tensor of `shape` in the middle of a flat sentinel-filled buffer"""

    def __init__(self, shape, f32):
        self.shape, self.f32 = tuple(shape), f32
        n = 1
        for s in shape:
            n *= s
        self.flat = self._sentinel(n + 2 * GUARD)
        self.view = self.flat[GUARD:GUARD + n].view(shape)

    def _sentinel(self, n):
        return torch.full((n,), NAN, dtype=torch.float32, device="cuda") if self.f32 else H.sentinel16((n,), ops.act_dtype(), "cuda")

    def expected(self, values, out_mode, out_off):
        """the whole buffer a correct launch leaves: `values` [B, OH, OW, Co] where it owns, the sentinel everywhere else"""
        e = self._sentinel(self.flat.numel())
        n = self.view.numel()
        e[GUARD:GUARD + n] = C.place(e[GUARD:GUARD + n].view(self.shape), values, out_mode, out_off).reshape(-1)
        return e


def _window(vals64, pitch, off, dtype=None):
    """[..., c] values -> channels [off, off + c) of a NaN-filled [..., pitch] device buffer of the 16-bit format (or `dtype`)"""
    dtype = dtype or ops.act_dtype()
    buf = torch.full(tuple(vals64.shape[:-1]) + (pitch,), NAN, dtype=dtype)
    buf[..., off:off + vals64.shape[-1]] = vals64.to(dtype)
    assert torch.equal(buf[..., off:off + vals64.shape[-1]].double(), vals64.double().cpu()), "operands are not numbers of the format"
    return buf.cuda()


def _twice(launch):
    first, second = launch(), launch()
    for a, b in zip(first, second):
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), "two runs of one launch differ"
    return first


def _dev(o):
    return {k: (None if v is None else v.cuda()) for k, v in o.items()}


def _check_bounded(got, exact, slack, tag):
    if got.dtype == torch.float32:
        return assert_f32(got.contiguous(), exact, slack, tag)
    return assert_rounded(got.contiguous(), exact, slack + C.binade_extra(exact, slack, ops.act_dtype()), tag)


def _stats_depth(parts_per_group):
    """additions behind one fused statistic: a part holds at most 4 rows x 32 pixels (one 32-row block of the weight-stationary kernel) x 4
    channels = 512 values however its lanes fold them; the reduce kernel's 256 threads chain their share of the parts, a wave folds in 6
    steps, 3 more join the waves; a square rounds once"""
    return 512 + -(-parts_per_group // 256) + 9 + 1


def _check_stats(stats, y_written, parts, tag):
    """the fused GroupNorm statistics against the fp64 sums of the output the kernel actually wrote (_GnStats.reduce's [B, 1, 32, 2])"""
    assert tuple(stats.shape) == (y_written.shape[0], 1, 32, 2) and stats.dtype == torch.float32
    exact, mags = C.gn_stats(y_written.double())
    upg = y_written.shape[-1] // 128
    assert_f32(stats, exact, _stats_depth(parts * upg) * U * mags, tag + ":stats")


# ---- (a) the implicit-GEMM kernel: every family, tile and epilogue ----------------------------------------------------------------------
@pytest.mark.parametrize("c", C.IGEMM_CASES, ids=[c["name"] for c in C.IGEMM_CASES])
def test_igemm_per_element(prec, c, ws_calls):
    dtype = ops.act_dtype()
    lay = C.case_layout(c)
    assert C.case_dispatch(c) == c["want"]
    family, tn, epi = c["want"]
    B, H_, W_ = c["B"], c["H"], c["W"]
    OH, OW = C.out_size(H_, W_, c["k"], c["stride"], c["ups"])
    f32 = c["mode"] in (C.NHWC32, C.PLANAR32)
    planar = c["mode"] in (C.PLANAR32, C.PLANAR16)
    shape = (B, lay["out_pitch"], lay["plane_pitch"]) if planar else (B, OH, OW, lay["out_pitch"])
    assert not planar or lay["plane_pitch"] > OH * OW
    for fam in ("int", "normal"):
        o = C.case_operands(c, fam, dtype)
        x = _window(o["x"], lay["in_pitch"], lay["in_off"])
        x2 = _window(o["x2"], lay["in2_pitch"], lay["in2_off"]) if c["cin2"] else None
        res = _window(o["res"], lay["res_pitch"], lay["res_off"]) if c["res"] else None
        bias = None if o["bias"] is None else o["bias"].float().cuda()
        pc = ops.PackedConv(o["w"].float().cuda(), bias, cout_tile=c["tile"], upsample_subpixel=c["subpixel"])
        assert pc.cout_tile == c["tile"] and pc.subpixel == c["subpixel"]

        def launch():
            out = _Out(shape, f32)
            r = ops.conv2d(x, pc, x2=x2, cin=c["cin"], in_off=lay["in_off"], cin2=c["cin2"] or None, in2_off=lay["in2_off"], stride=c["stride"],
                           upsample=c["ups"], act=c["act"], residual=res, res_off=lay["res_off"], out=out.view, out_off=lay["out_off"],
                           out_mode=c["mode"], gn_stats=c["stats"])
            assert r is out.view
            launch.out = out
            return out.flat, getattr(r, "_gn_stats", None)
        flat, stats = _twice(launch)
        out = launch.out
        ref = C.case_reference(c, _dev(o), dtype)
        tag = "%s:%s:%s" % (family, epi, c["name"])
        if fam == "int":
            if c["act"] in ("sigmoid", "swish"):
                continue          # the activation's own evaluation rounds: BOUNDED only
            want = ref.value(c["act"]) if (f32 or epi != "fast") else C.staged16(ref, c["act"], dtype)
            assert float(want.abs().max()) <= C.LIMIT[torch.float32 if f32 else dtype]
            H.assert_same_bits(flat, out.expected(want, c["mode"], lay["out_off"]), tag + " EQUAL")
        else:
            got = C.owned(out.view, (B, OH, OW, c["cout"]), c["mode"], lay["out_off"])
            exact, slack = C.case_bound(c, ref, dtype)
            _check_bounded(got, exact, slack, tag)
            H.assert_same_bits(flat, out.expected(got.double(), c["mode"], lay["out_off"]), tag + " outside its window")
        if c["stats"]:
            got = C.owned(out.view, (B, OH, OW, c["cout"]), c["mode"], lay["out_off"])
            src_h, src_w = (H_, W_) if c["subpixel"] else (OH, OW)
            parts = -(-src_w // C.TILE_COLS) * -(-src_h // C.TILE_ROWS) * 2 * (4 if c["subpixel"] else 1)
            _check_stats(stats, got, parts, tag + ":" + fam)
    assert not ws_calls, "an implicit-GEMM case went to the weight-stationary kernel"


def test_subpixel_feedback_filters(prec):
    """PackedConv(upsample_subpixel=True, feedback=True): the four phase filters rounded by the error-feedback definition (conv_fp64.
    feedback_round on the exact phase sums: 16-bit taps within 2^-10 .. 1 sum exactly in fp32 in any order), then the same conv"""
    dtype = ops.act_dtype()
    gen = torch.Generator().manual_seed(41)
    B, H_, W_, cin, cout = 2, 5, 33, 24, 40
    x64, w64 = C.normal_operands(gen, (B, H_, W_, cin), (cout, cin, 3, 3), dtype)
    bias = torch.randn(cout, generator=gen) * 0.25
    x = _window(x64, cin + 16, 8)
    pc = ops.PackedConv(w64.float().cuda(), bias.cuda(), upsample_subpixel=True, feedback=True)
    ph = C.subpixel_filters(w64)
    assert torch.equal(ph.float().double(), ph)
    ph = C.feedback_round(ph.reshape(4 * cout, cin, 2, 2), dtype).reshape(4, cout, cin, 2, 2).cuda()
    assert C.igemm_dispatch(3, 1, True, cout, 0, C.NHWC16, cout + 16, 8, False, 0, 0, "none") == ("k2", 64, "fast")

    def launch():
        out = _Out((B, 2 * H_, 2 * W_, cout + 16), False)
        ops.conv2d(x, pc, cin=cin, in_off=8, upsample=True, out=out.view, out_off=8)
        launch.out = out
        return (out.flat,)
    (flat,) = _twice(launch)
    acc, mag = C.subpixel_conv(x64.cuda(), ph), C.subpixel_conv(x64.cuda().abs(), ph.abs())
    b64 = bias.double().cuda()
    got = launch.out.view[..., 8:8 + cout]
    _check_bounded(got, acc + b64, C.mfma_slack(C.padded_k(3, cin, True), mag) + 2 * U * (mag + b64.abs()), "k2:feedback")
    H.assert_same_bits(flat, launch.out.expected(got.double(), C.NHWC16, 8), "k2 feedback outside its window")


# ---- (b) grouped launches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", (1, 5))
@pytest.mark.parametrize("k,cin,cout,out_step,mode", ((3, 16, 6, 8, C.NHWC32), (1, 32, 64, 72, C.NHWC16)))
def test_grouped_launch_per_element(prec, G, k, cin, cout, out_step, mode, ws_calls):
    """glare_conv_desc.groups: group g reads channels [in_off + g in_step, + cin), writes [out_off + g out_step, + cout); the gaps of
    out_step > cout keep the sentinel, the gaps of in_step > cin are NaN"""
    dtype = ops.act_dtype()
    B, H_, W_, in_step, in_off, out_off = 2, 9, 33, cin + 8, 8, 8
    f32 = mode == C.NHWC32
    fam_want = C.igemm_dispatch(k, 1, False, cout, 0, mode, out_off + G * out_step, out_off, False, 0, 0, "relu")
    assert fam_want == (("k3s1", 32, "general") if f32 else ("k1", 64, "fast"))
    for fam in ("int", "normal"):
        gen = torch.Generator().manual_seed(G * 100 + k + (fam == "int"))
        xs, ws, bs = [], [], []
        for _ in range(G):
            x64, w64 = C.int_operands(gen, (B, H_, W_, cin), (cout, cin, k, k)) if fam == "int" else C.normal_operands(gen, (B, H_, W_, cin), (cout, cin, k, k), dtype)
            xs.append(x64), ws.append(w64), bs.append(C.int_bias(gen, cout) if fam == "int" else (torch.randn(cout, generator=gen) * 0.25).float().double())
        xbuf = torch.full((B, H_, W_, in_off + G * in_step), NAN, dtype=dtype)
        for g in range(G):
            xbuf[..., in_off + g * in_step:in_off + g * in_step + cin] = xs[g].to(dtype)
        xbuf = xbuf.cuda()
        pcs = ops.packed_conv_batch(torch.stack(ws).float().cuda(), torch.stack(bs).float().cuda())

        def launch():
            out = _Out((B, H_, W_, out_off + G * out_step), f32)
            ops.conv2d_grouped(xbuf, pcs, cin=cin, in_step=in_step, in_off=in_off, out=out.view, out_step=out_step, out_off=out_off, act="relu",
                               out_mode=mode)
            launch.out = out
            return (out.flat,)
        (flat,) = _twice(launch)
        out = launch.out
        e = out._sentinel(out.flat.numel())
        ev = e[GUARD:GUARD + out.view.numel()].view(out.shape)
        for g in range(G):
            acc, mag = C.conv_acc(xs[g].cuda(), ws[g].cuda()), C.conv_acc(xs[g].cuda().abs(), ws[g].cuda().abs())
            b64 = bs[g].cuda()
            lo = out_off + g * out_step
            if fam == "int":
                assert float((acc + b64).abs().max()) <= C.LIMIT[torch.float32 if f32 else dtype]
                ev[..., lo:lo + cout] = (acc + b64).clamp_min(0).to(ev.dtype)
            else:
                _check_bounded(out.view[..., lo:lo + cout], (acc + b64).clamp_min(0), C.mfma_slack(C.padded_k(k, cin), mag) + 2 * U * (mag + b64.abs()),
                               "grouped:k%d:G%d" % (k, G))
                ev[..., lo:lo + cout] = out.view[..., lo:lo + cout]
        H.assert_same_bits(flat, e, "grouped k%d G%d: %s" % (k, G, "EQUAL" if fam == "int" else "outside its windows"))
    assert not ws_calls


# ---- (c) the data-gradient pack ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,co,ci,P", ((3, 24, 16, 32), (1, 40, 72, 64)))
def test_dgrad_pack_is_the_input_gradient(prec, k, co, ci, P, ws_calls):
    """PackedConv(w, dgrad_pad=P) then the same conv == conv_acc(g padded to P channels, dgrad_filter(w)): the fp64 gradient of F.conv2d with
    respect to its input (test_conv_fp64_host.py); P > cout, the padded channels of g are zero"""
    dtype = ops.act_dtype()
    B, H_, W_ = 2, 9, 33
    for fam in ("int", "normal"):
        gen = torch.Generator().manual_seed(k * 10 + (fam == "int"))
        g64, w64 = (C.int_operands(gen, (B, H_, W_, co), (co, ci, k, k)) if fam == "int" else C.normal_operands(gen, (B, H_, W_, co), (co, ci, k, k), dtype))
        if fam == "int":          # the contraction runs over co k k: the density of that K
            w64 = w64.sign() * (torch.rand(w64.shape, generator=gen) < C.int_density(co * k * k)).double() if co * k * k > 64 else w64
        gpad = torch.cat([g64, torch.zeros(B, H_, W_, P - co, dtype=torch.float64)], -1)
        gbuf = _window(gpad, P + 16, 8)
        pc = ops.PackedConv(w64.float().cuda(), None, dgrad_pad=P)
        assert (pc.ksize, pc.cout, pc.cin, pc.w16) == (k, ci, P, None)
        want_family = C.igemm_dispatch(k, 1, False, ci, 0, C.NHWC16, ci + 16, 8, False, 0, 0, "none")
        assert want_family == (("k3s1", 32, "fast") if k == 3 else ("k1", 128, "fast"))

        def launch():
            out = _Out((B, H_, W_, ci + 16), False)
            ops.conv2d(gbuf, pc, cin=P, in_off=8, out=out.view, out_off=8)
            launch.out = out
            return (out.flat,)
        (flat,) = _twice(launch)
        wd = C.dgrad_filter(w64, P).cuda()
        acc, mag = C.conv_acc(gpad.cuda(), wd), C.conv_acc(gpad.cuda().abs(), wd.abs())
        if fam == "int":
            assert float(acc.abs().max()) <= C.LIMIT[dtype]
            H.assert_same_bits(flat, launch.out.expected(acc, C.NHWC16, 8), "dgrad k%d EQUAL" % k)
        else:
            got = launch.out.view[..., 8:8 + ci]
            _check_bounded(got, acc, C.mfma_slack(C.padded_k(k, P), mag), "dgrad:k%d" % k)
            H.assert_same_bits(flat, launch.out.expected(got.double(), C.NHWC16, 8), "dgrad outside its window")
    assert not ws_calls


# ---- (d) hi / lo outputs and the fp32-class form on the implicit-GEMM kernel ------------------------------------------------------------
def _pair_window(hi64, lo64, pitch, off):
    x = _window(hi64, pitch, off)
    x._lo = _window(lo64, pitch, off)
    return x


def _split16(v32, dtype):
    hi = v32.to(dtype)
    return hi.double(), (v32 - hi.float()).to(dtype).double()


# (name, k, stride, cin, cout, pair residual, pair output (else fp32), split (else a single-pass filter), expected family)
HILO_CASES = (
    ("k3s1 split pair res", 3, 1, 32, 128, True, True, True, ("k3s1", 128, "hilo")),
    ("k3s2 split pair", 3, 2, 16, 128, False, True, True, ("k3s2", 128, "hilo")),
    ("k1 split pair 128", 1, 1, 64, 128, True, True, True, ("k1", 128, "hilo")),
    ("k1 split pair 64", 1, 1, 64, 64, False, True, True, ("k1", 64, "hilo")),
    ("k3s1 split fp32", 3, 1, 32, 40, False, False, True, ("k3s1", 64, "general")),
    ("k3s1 single pass pair", 3, 1, 24, 128, True, True, False, ("k3s1", 128, "hilo")),
)


HILO_PARAMS = [(c, reuse) for c in HILO_CASES for reuse in ((True, False) if c[7] else (True,))]          # a single-pass filter has one K order


@pytest.mark.parametrize("case,reuse", HILO_PARAMS, ids=["%s-%s" % (c[0], "reuse" if r else "segments") for c, r in HILO_PARAMS])
def test_hilo_and_split_per_element(prec, case, reuse, monkeypatch, ws_calls):
    """The HILO instantiations and the fp32-class K segments (both k_wrap orders: SPLIT_A_REUSE).  v = acc + bias + residual_hi +
    residual_lo in fp32, nothing rounded before the residual add; hi = round16(v), lo = round16(v - hi).  Integer operands have zero lo
    halves: hi must EQUAL the fp64 value, lo must be +0.  Normal operands: the three products of conv_fp64.split3 on Kp = padded 3 cin
    k k MFMA products, the dropped sum |x_lo| |w_lo| as its own term, one addition each for bias, residual_hi and residual_lo."""
    name, k, stride, cin, cout, pres, pout, split, want = case
    monkeypatch.setattr(ops, "SPLIT_A_REUSE", reuse)
    dtype = ops.act_dtype()
    B, H_, W_ = 2, 9, 33
    OH, OW = C.out_size(H_, W_, k, stride, False)
    assert C.igemm_dispatch(k, stride, False, cout, 0, C.NHWC16 if pout else C.NHWC32, cout, 0, pres, cout + 16, 8, "none", hilo=pout) == want
    assert not C.ws_supported(cin, cout, split=True)
    for fam in ("int", "normal"):
        gen = torch.Generator().manual_seed(sum(map(ord, name)) + (fam == "int"))
        if fam == "int":
            xh, w64 = C.int_operands(gen, (B, H_, W_, cin), (cout, cin, k, k))
            xl = torch.zeros_like(xh)
            b64 = C.int_bias(gen, cout)
            rh, rl = C.int_residual(gen, (B, OH, OW, cout)), torch.zeros(B, OH, OW, cout, dtype=torch.float64)
        else:
            K = cin * k * k
            xh, xl = _split16(torch.randn(B, H_, W_, cin, generator=gen), dtype)
            w64 = (torch.randn(cout, cin, k, k, generator=gen) / K ** 0.5).double()
            if not split:
                w64 = w64.float().to(dtype).double()
            b64 = (torch.randn(cout, generator=gen) * 0.25).float().double()
            rh, rl = _split16(torch.randn(B, OH, OW, cout, generator=gen), dtype)
        x = _pair_window(xh, xl, cin + 16, 8) if split else _window(xh, cin + 16, 8)
        res = _pair_window(rh, rl, cout + 16, 8) if pres else None
        pc = ops.PackedConv(w64.float().cuda(), b64.float().cuda(), split=3 if split else 0)
        assert pc.k_wrap == ((2 if reuse and k == 3 and cin % 16 == 0 else 1) if split else 0)

        def launch():
            out = _Out((B, OH, OW, cout), not pout)
            if pout:
                lo = _Out((B, OH, OW, cout), False)
                out.view._lo = lo.view
            r = ops.conv2d(x, pc, cin=cin, in_off=8, stride=stride, residual=res, res_off=8, out=out.view, hilo=pout,
                           out_mode=C.NHWC16 if pout else C.NHWC32)
            assert r is out.view and (not pout or r._lo is lo.view)
            launch.out = out
            return out.flat, (lo.flat if pout else None)
        flat, loflat = _twice(launch)
        out = launch.out
        d = lambda t: t.cuda()
        if split:
            acc, mag, dropped = C.split3(d(xh), d(xl), d(w64), dtype, stride)
            kp = C.padded_k(k, 3 * cin)
        else:
            acc, mag, dropped = C.conv_acc(d(xh), d(w64), stride), C.conv_acc(d(xh).abs(), d(w64).abs(), stride), 0.0
            kp = C.padded_k(k, cin)
        exact = acc + d(b64) + ((d(rh) + d(rl)) if pres else 0.0)
        mags = mag + d(b64).abs() + ((d(rh).abs() + d(rl).abs()) if pres else 0.0)
        if fam == "int":
            assert float(exact.abs().max()) <= C.LIMIT[dtype]
            H.assert_same_bits(flat, out.expected(exact, C.NHWC16 if pout else C.NHWC32, 0), name + " EQUAL")
            if pout:
                H.assert_same_bits(loflat, out.expected(torch.zeros_like(exact), C.NHWC16, 0), name + " lo of an exact value is +0")
            continue
        slack = C.mfma_slack(kp, mag) + dropped + 2 * U * mags * (3 if pres else 1)
        tag = "%s:%s" % (name, "reuse" if reuse else "segments")
        _check_bounded(out.view, exact, slack, tag + ":hi")
        if pout:
            value = out.view.double() + out.view._lo.double()
            within(float(((value - exact).abs() / (slack + C.pair_slack(exact, slack, dtype))).max()), 1.0, "%s:%s:pair" % (ops.precision(), tag))
            # lo is the rounding of v - hi for the v the kernel held: within half an ulp16 of hi's remainder, and hi is v's nearest
            assert bool((out.view._lo.double().abs() <= 0.5 * C.ulp16(out.view.double(), dtype) * (1 + 2.0 ** -7)).all())
        for f in (flat, loflat):          # the guards in front of and behind a tensor the launch owns whole
            if f is not None:
                guard = _bits(out._sentinel(GUARD) if f is flat else H.sentinel16((GUARD,), dtype, "cuda"))
                assert torch.equal(_bits(f[:GUARD]), guard) and torch.equal(_bits(f[-GUARD:]), guard), name + " wrote outside its tensor"
    assert not ws_calls


# ---- (e) the GroupNorm prologue ----------------------------------------------------------------------------------------------------------
def test_groupnorm_prologue_per_element(prec, ws_calls):
    """glare_conv_desc.gn_coef against round16(act(a x + d)) followed by the conv, the zero padding staying zero.  EQUAL: a in {1, 2, -2}, d in
    {-1, 0, 1}, x = +-1, no swish -- a x + d is an exact integer, so are the sums.  BOUNDED (swish): the normalised operand is round16 of
    an fp32 evaluation; an element whose fp64 value lies within that evaluation's error of a rounding tie may land on the other
    neighbour, one ulp16 away: sum |w| ulp16 over exactly those elements is added to the MFMA chain's slack."""
    dtype = ops.act_dtype()
    B, H_, W_, cin, cout = 2, 9, 33, 32, 128
    kp = C.padded_k(3, cin)
    assert C.igemm_dispatch(3, 1, False, cout, 0, C.NHWC16, cout + 16, 8, False, 0, 0, "none", gnp=True) == ("k3s1", 128, "gnp")
    for fam in ("int", "normal"):
        gen = torch.Generator().manual_seed(7 + (fam == "int"))
        if fam == "int":
            x64 = C._signs(gen, (B, H_, W_, cin))
            a = torch.tensor([1.0, 2.0, -2.0])[torch.randint(0, 3, (B, cin), generator=gen)].double()
            dd = torch.randint(-1, 2, (B, cin), generator=gen).double()
            w64 = C._signs(gen, (cout, cin, 3, 3)) * (torch.rand(cout, cin, 3, 3, generator=gen) < C.int_density(9 * cin, 3.0 + 2.0 / 3.0)).double()
            b64 = C.int_bias(gen, cout)
        else:
            x64, w64 = C.normal_operands(gen, (B, H_, W_, cin), (cout, cin, 3, 3), dtype)
            a = (1.0 + 0.3 * torch.randn(B, cin, generator=gen)).float().double()
            dd = (0.2 * torch.randn(B, cin, generator=gen)).float().double()
            b64 = (torch.randn(cout, generator=gen) * 0.25).float().double()
        swish = fam == "normal"
        x = _window(x64, cin + 8, 0)
        coef = torch.stack([a, dd], -1).float().cuda()
        pc = ops.PackedConv(w64.float().cuda(), b64.float().cuda())

        def launch():
            out = _Out((B, H_, W_, cout + 16), False)
            ops.conv2d(x, pc, cin=cin, out=out.view, out_off=8, gn_prologue=(coef, swish))
            launch.out = out
            return (out.flat,)
        (flat,) = _twice(launch)
        u = x64 * a.view(B, 1, 1, cin) + dd.view(B, 1, 1, cin)
        n64 = C.act64(u, "swish" if swish else "none")
        n16 = n64.to(dtype).double()
        acc, mag = C.conv_acc(n16.cuda(), w64.cuda()), C.conv_acc(n16.cuda().abs(), w64.cuda().abs())
        if fam == "int":
            assert torch.equal(n16, n64) and float((acc + b64.cuda()).abs().max()) <= C.LIMIT[dtype]
            assert float((n64 == 0).double().mean()) < 0.5
            H.assert_same_bits(flat, launch.out.expected(acc + b64.cuda(), C.NHWC16, 8), "gn prologue EQUAL")
            continue
        e_u = 2 * U * ((x64 * a.view(B, 1, 1, cin)).abs() + dd.view(B, 1, 1, cin).abs())
        e_n = C.act_slack(u, e_u, "swish")
        to_tie = 0.5 * C.ulp16(n64, dtype) - (n64 - n16).abs()
        flip = (to_tie <= e_n).double() * C.ulp16(n64.abs() + e_n, dtype)
        slack = C.mfma_slack(kp, mag) + 2 * U * (mag + b64.cuda().abs()) + C.conv_acc(flip.cuda(), w64.cuda().abs())
        got = launch.out.view[..., 8:8 + cout]
        _check_bounded(got, acc + b64.cuda(), slack, "gn prologue:swish")
        H.assert_same_bits(flat, launch.out.expected(got.double(), C.NHWC16, 8), "gn prologue outside its window")
    assert not ws_calls


# ---- (f) the weight-stationary 1x1 kernel ------------------------------------------------------------------------------------------------
# (B, H, W, cin, cout, residual, act, fused statistics): pixels per image 1, 31, 32, 33, 100; more images than the 32 pixel ranges of 8
# co-tiles have row blocks; row blocks that end inside an image
WS_CASES = ((1, 1, 1, 128, 128, False, "none", False), (2, 1, 31, 256, 256, True, "relu", False), (3, 4, 8, 512, 512, False, "relu", False),
            (9, 3, 11, 128, 1024, True, "none", False), (2, 10, 10, 128, 256, True, "none", True), (2, 3, 11, 512, 128, False, "none", True))


def _ws_operands(gen, fam, B, H_, W_, cin, cout, dtype):
    if fam == "int":
        x64, w64 = C.int_operands(gen, (B, H_, W_, cin), (cout, cin, 1, 1))
        return x64, w64, C.int_bias(gen, cout), C.int_residual(gen, (B, H_, W_, cout))
    x64, w64 = C.normal_operands(gen, (B, H_, W_, cin), (cout, cin, 1, 1), dtype)
    return x64, w64, (torch.randn(cout, generator=gen) * 0.25).float().double(), C.normal16(gen, (B, H_, W_, cout), dtype)


def _staged_bound(acc, mag, b64, r64, act, kp, dtype):
    """the plain epilogue of the weight-stationary kernel is the LDS-staged one: conv_fp64.case_bound's count"""
    ref = C.Ref(acc, mag, b64, torch.zeros_like(acc) if r64 is None else r64, r64 is not None)
    e = C.mfma_slack(kp, mag) + 2 * U * ref.mag_all()
    if r64 is not None:
        e = e + 0.5 * C.ulp16((acc + b64).abs() + e, dtype) + 2 * U * ref.mag_all()
    return ref, ref.value(act), e


@pytest.mark.parametrize("case", WS_CASES, ids=["x".join(str(v) for v in c[:5]) for c in WS_CASES])
def test_ws_plain_per_element(prec, case, ws_calls):
    B, H_, W_, cin, cout, with_res, act, stats = case
    dtype = ops.act_dtype()
    assert C.ws_supported(cin, cout)
    for fam in ("int", "normal"):
        gen = torch.Generator().manual_seed(B * 1000 + H_ * W_ + cin + cout + (fam == "int"))
        x64, w64, b64, r64 = _ws_operands(gen, fam, B, H_, W_, cin, cout, dtype)
        x = _window(x64, cin + 16, 8)
        res = _window(r64, cout + 24, 16) if with_res else None
        pc = ops.PackedConv(w64.float().cuda(), b64.float().cuda())
        assert pc.w16 is not None
        del ws_calls[:]

        def launch():
            if stats:          # fused statistics only into an output of the launch's own (_ws_eligible)
                r = ops.conv2d(x, pc, cin=cin, in_off=8, act=act, residual=res, res_off=16, gn_stats=True)
                return r, r._gn_stats
            out = _Out((B, H_, W_, cout + 16), False)
            assert ops._ws_eligible(pc, x, cin, 8, None, 1, False, C.NHWC16, out.view, 8, res, 16, False, False, None)
            ops.conv2d(x, pc, cin=cin, in_off=8, act=act, residual=res, res_off=16, out=out.view, out_off=8)
            launch.out = out
            return out.flat, None
        flat, st = _twice(launch)
        assert len(ws_calls) == 2, "the launch did not take the weight-stationary kernel"
        acc, mag = C.conv_acc(x64.cuda(), w64.cuda()), C.conv_acc(x64.cuda().abs(), w64.cuda().abs())
        ref, exact, slack = _staged_bound(acc, mag, b64.cuda(), r64.cuda() if with_res else None, act, cin, dtype)
        got = flat if stats else launch.out.view[..., 8:8 + cout]
        tag = "ws:%s" % "x".join(str(v) for v in case[:5])
        if fam == "int":
            want = C.staged16(ref, act, dtype)
            assert float(want.abs().max()) <= C.LIMIT[dtype]
            if stats:
                H.assert_same_bits(got, want.to(dtype), tag + " EQUAL")
            else:
                H.assert_same_bits(flat, launch.out.expected(want, C.NHWC16, 8), tag + " EQUAL")
        else:
            _check_bounded(got, exact, slack, tag)
            if not stats:
                H.assert_same_bits(flat, launch.out.expected(got.double(), C.NHWC16, 8), tag + " outside its window")
        if stats:
            _check_stats(st, got, -(-H_ * W_ // 32), tag + ":" + fam)


@pytest.mark.parametrize("B,cin,cout,pres", ((2, 128, 128, True), (3, 256, 256, False)))
def test_ws_hilo_per_element(prec, B, cin, cout, pres, ws_calls):
    """glare_conv1x1_ws_hilo_bf16 through conv2d(hilo=True) on a single-pass 1x1 filter: v = acc + bias + (residual_hi + residual_lo)"""
    dtype = ops.act_dtype()
    H_, W_ = 3, 11
    for fam in ("int", "normal"):
        gen = torch.Generator().manual_seed(B + cin + (fam == "int"))
        x64, w64, b64, r64 = _ws_operands(gen, fam, B, H_, W_, cin, cout, dtype)
        rl64 = torch.zeros_like(r64) if fam == "int" else _split16(torch.randn(r64.shape, generator=gen) * 2.0 ** -9, dtype)[0]
        x = _window(x64, cin + 16, 8)
        res = _pair_window(r64, rl64, cout + 8, 8) if pres else None
        pc = ops.PackedConv(w64.float().cuda(), b64.float().cuda())

        def launch():
            r = ops.conv2d(x, pc, cin=cin, in_off=8, residual=res, res_off=8, hilo=True)
            return r, r._lo
        hi, lo = _twice(launch)
        acc, mag = C.conv_acc(x64.cuda(), w64.cuda()), C.conv_acc(x64.cuda().abs(), w64.cuda().abs())
        exact = acc + b64.cuda() + ((r64 + rl64).cuda() if pres else 0.0)
        mags = mag + b64.cuda().abs() + ((r64.abs() + rl64.abs()).cuda() if pres else 0.0)
        if fam == "int":
            assert float(exact.abs().max()) <= C.LIMIT[dtype]
            H.assert_same_bits(hi, exact.to(dtype), "ws hilo EQUAL")
            H.assert_same_bits(lo, torch.zeros_like(hi), "ws hilo: lo of an exact value is +0")
        else:
            slack = C.mfma_slack(cin, mag) + 2 * U * mags * (3 if pres else 1)
            _check_bounded(hi, exact, slack, "ws:hilo:%d" % cin)
            within(float((((hi.double() + lo.double()) - exact).abs() / (slack + C.pair_slack(exact, slack, dtype))).max()), 1.0,
                   "%s:ws:hilo:%d:pair" % (ops.precision(), cin))
    assert len(ws_calls) == 4


@pytest.mark.parametrize("B,cin,cout,pout,pres", ((2, 128, 64, True, True), (3, 256, 128, False, False), (1, 512, 256, True, False)))
def test_ws_split_per_element(prec, B, cin, cout, pout, pres, ws_calls):
    """glare_conv1x1_ws_split_bf16: the LDS image holds w_hi and w_lo of the same 64 output channels; acc0 chains x_hi w_hi and x_lo w_hi (2
    cin products), acc2 x_hi w_lo, (acc0 + acc2) + bias: counted as the 3 cin products of the segment form plus one addition"""
    dtype = ops.act_dtype()
    H_, W_ = 3, 11
    assert C.ws_supported(cin, cout, split=True)
    for fam in ("int", "normal"):
        gen = torch.Generator().manual_seed(B + cin + cout + (fam == "int"))
        if fam == "int":
            xh, w64, b64, rh = _ws_operands(gen, fam, B, H_, W_, cin, cout, dtype)
            xl, rl = torch.zeros_like(xh), torch.zeros_like(rh)
        else:
            xh, xl = _split16(torch.randn(B, H_, W_, cin, generator=gen), dtype)
            w64 = (torch.randn(cout, cin, 1, 1, generator=gen) / cin ** 0.5).double()
            b64 = (torch.randn(cout, generator=gen) * 0.25).float().double()
            rh, rl = _split16(torch.randn(B, H_, W_, cout, generator=gen), dtype)
        x = _pair_window(xh, xl, cin + 16, 8)
        res = _pair_window(rh, rl, cout + 8, 8) if pres else None
        pc = ops.PackedConv(w64.float().cuda(), b64.float().cuda(), split=3)
        assert pc.w16_lo is not None
        assert ops._ws_eligible(pc, x, cin, 8, None, 1, False, C.NHWC16, None, 0, res, 8, False, pout, None)

        def launch():
            r = ops.conv2d(x, pc, cin=cin, in_off=8, residual=res, res_off=8, hilo=pout)
            return r, getattr(r, "_lo", None)
        hi, lo = _twice(launch)
        assert (lo is not None) == pout
        acc, mag, dropped = C.split3(xh.cuda(), xl.cuda(), w64.cuda(), dtype)
        exact = acc + b64.cuda() + ((rh + rl).cuda() if pres else 0.0)
        mags = mag + b64.cuda().abs() + ((rh.abs() + rl.abs()).cuda() if pres else 0.0)
        if fam == "int":
            assert float(exact.abs().max()) <= C.LIMIT[dtype]
            H.assert_same_bits(hi, exact.to(dtype), "ws split EQUAL")
            if pout:
                H.assert_same_bits(lo, torch.zeros_like(hi), "ws split: lo of an exact value is +0")
        else:
            slack = C.mfma_slack(3 * cin, mag) + dropped + 2 * U * mags * (4 if pres else 2)
            _check_bounded(hi, exact, slack, "ws:split:%d" % cin)
            if pout:
                within(float((((hi.double() + lo.double()) - exact).abs() / (slack + C.pair_slack(exact, slack, dtype))).max()), 1.0,
                       "%s:ws:split:%d:pair" % (ops.precision(), cin))
    assert len(ws_calls) == 4


@pytest.mark.parametrize("B", (1, 2, 4))
def test_ws_per_image_filters(prec, B):
    """conv1x1_per_image: image b against its own [Cout, Cin] filter and bias (+ residual, fused statistics): a pixel range that took the
    neighbouring image's filter or bias changes every element"""
    dtype = ops.act_dtype()
    H_, W_, cin, cout = 3, 11, 128, 256
    for fam in ("int", "normal"):
        gen = torch.Generator().manual_seed(B + (fam == "int"))
        per = [_ws_operands(gen, fam, 1, H_, W_, cin, cout, dtype) for _ in range(B)]
        x = torch.cat([p[0] for p in per]).to(dtype).cuda()
        w16 = torch.stack([p[1].view(cout, cin) for p in per]).to(dtype).cuda()
        bias = torch.stack([p[2] for p in per]).float().cuda()
        res = torch.cat([p[3] for p in per]).to(dtype).cuda()

        def launch():
            r = ops.conv1x1_per_image(x, w16, bias, residual=res, gn_stats=True)
            return r, r._gn_stats
        got, st = _twice(launch)
        for b, (x64, w64, b64, r64) in enumerate(per):
            acc, mag = C.conv_acc(x64.cuda(), w64.cuda()), C.conv_acc(x64.cuda().abs(), w64.cuda().abs())
            ref, exact, slack = _staged_bound(acc, mag, b64.cuda(), r64.cuda(), "none", cin, dtype)
            if fam == "int":
                H.assert_same_bits(got[b:b + 1], C.staged16(ref, "none", dtype).to(dtype), "per-image EQUAL image %d of %d" % (b, B))
            else:
                _check_bounded(got[b:b + 1], exact, slack, "ws:per-image:%d" % B)
        _check_stats(st, got, -(-H_ * W_ // 32), "ws:per-image:%d:%s" % (B, fam))


# ---- (g) conv_small ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,cin", ((1, 1), (1, 3), (1, 4), (3, 1), (3, 3), (3, 4)))
def test_smallcin_per_element(prec, k, cin):
    """conv2d_smallcin: fp32 operands through element strides (NCHW planes; NHWC records with two foreign NaN channels), an fp32 FMA chain
    that starts at the bias: one rounding per FMA, k k cin of them, counted as (k k cin + 1) U sum |terms| with the bias among the terms;
    integers are exact through FMA and through separate multiply and add alike.  Cout 64 with cin 3, k 3 takes the LDS-staged kernel (groups a power
    of two in 8 .. 64), every other shape the generic one.  W in {1, 3, 4, 5, 9}: the 4-pixels-per-lane tail."""
    dtype = ops.act_dtype()
    B, H_ = 2, 3
    n = 0
    for cout in (3, 8, 64, 136):
        for W_ in (1, 3, 4, 5, 9):
            layout = ("nchw", "nhwc")[n % 2]
            kind = ("f32", "16", "pair")[n % 3] if cout % 8 == 0 else ("f32", "16")[n % 2]
            n += 1
            for fam in ("int", "normal"):
                gen = torch.Generator().manual_seed(cout * 100 + W_ * 10 + k + cin + (fam == "int"))
                if fam == "int":
                    x64, w64 = C.int_operands(gen, (B, H_, W_, cin), (cout, cin, k, k))
                    b64 = C.int_bias(gen, cout)
                else:
                    x64 = torch.randn(B, H_, W_, cin, generator=gen).double()
                    w64 = (torch.randn(cout, cin, k, k, generator=gen) / (cin * k * k) ** 0.5).double()
                    b64 = (torch.randn(cout, generator=gen) * 0.25).double()
                if layout == "nchw":
                    xd = torch.full((16 + B * cin * H_ * W_ + 16,), NAN)
                    xd[16:-16] = x64.permute(0, 3, 1, 2).reshape(-1).float()
                    xd = xd.cuda()
                    xarg, strides = xd[16:], (cin * H_ * W_, H_ * W_, W_, 1)
                else:
                    rec = torch.full((B, H_, W_, cin + 2), NAN)
                    rec[..., 1:1 + cin] = x64.float()
                    xd = rec.cuda()
                    xarg, strides = xd.view(-1)[1:], (H_ * W_ * (cin + 2), 1, W_ * (cin + 2), cin + 2)
                w, b = w64.float().cuda(), b64.float().cuda()
                pitch, off = ((cout + 16, 8) if cout % 8 == 0 else (cout + 7, 3))

                def launch():
                    if kind == "pair":
                        r = ops.conv2d_smallcin(xarg, strides, (B, H_, W_), w, b, hilo=True)
                        return r, r._lo
                    out = _Out((B, H_, W_, pitch), kind == "f32")
                    ops.conv2d_smallcin(xarg, strides, (B, H_, W_), w, b, out=out.view, out_off=off, out_f32=kind == "f32")
                    launch.out = out
                    return out.flat, None
                first, lo = _twice(launch)
                ref = C.smallcin(xarg.double(), strides, B, H_, W_, w.double(), b.double())
                exact, slack = ref.pre(), (k * k * cin + 1) * U * ref.mag_all()
                mode = C.NHWC32 if kind == "f32" else C.NHWC16
                tag = "small:k%d:cin%d:%s" % (k, cin, kind)
                if kind == "pair":
                    if fam == "int":
                        H.assert_same_bits(first, exact.to(dtype), tag + " EQUAL")
                        H.assert_same_bits(lo, torch.zeros_like(first), tag + ": lo of an exact value is +0")
                    else:
                        _check_bounded(first, exact, slack, tag + ":hi")
                        within(float(((first.double() + lo.double() - exact).abs() / (slack + C.pair_slack(exact, slack, dtype))).max()), 1.0,
                               "%s:%s:pair" % (ops.precision(), tag))
                elif fam == "int":
                    H.assert_same_bits(first, launch.out.expected(exact, mode, off), tag + " EQUAL")
                else:
                    got = launch.out.view[..., off:off + cout]
                    _check_bounded(got, exact, slack, tag)
                    H.assert_same_bits(first, launch.out.expected(got.double(), mode, off), tag + " outside its window")


# ---- (h) refusals --------------------------------------------------------------------------------------------------------------------------
def test_conv2d_refuses_before_any_launch(prec):
    """Every GLARE_ERR_INVALID / GLARE_ERR_UNSUPPORTED branch of glare_conv2d_bf16 that no other test reaches: the status comes back and the
    sentinel output is untouched.  (The sub-pixel form under stride 2 or with an fp32 output, sigmoid / swish with fused statistics or the
    sub-pixel form, the 32-wide tile with fused statistics, a group past the pitch and the k_wrap rules: test_gpu_conv.py,
    test_gpu_split_conv.py.)  The residual's and the second source's windows, and negative offsets, were not checked on the parent commit."""
    dt = ops.act_dtype()
    x = torch.ones(2, 4, 4, 32, dtype=dt, device="cuda")
    res = torch.ones(2, 4, 4, 40, dtype=dt, device="cuda")
    coef = torch.ones(2, 16, 2, device="cuda")
    pc = ops.PackedConv(torch.ones(32, 16, 3, 3, device="cuda"), None)
    out = _Out((2, 4, 4, 40), False)
    lo = _Out((2, 4, 4, 40), False)
    lib = _lib.lib()
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED

    def base():
        d = ops.ConvDesc()
        d.in_, d.B, d.H, d.W, d.Cin, d.in_pitch, d.in_off = x.data_ptr(), 2, 4, 4, 16, 32, 8
        d.out, d.Cout, d.out_pitch, d.out_off = out.view.data_ptr(), 32, 40, 8
        d.weight_packed, d.ksize, d.stride, d.out_mode = pc.packed.data_ptr(), 3, 1, C.NHWC16
        return d

    def with_(**kw):
        d = base()
        for name, v in kw.items():
            setattr(d, name, v)
        return d
    R, X2, LO = res.data_ptr(), x.data_ptr(), lo.view.data_ptr()
    table = [
        (with_(in_=None), INV), (with_(weight_packed=None), INV), (with_(out=None), INV), (with_(B=0), INV), (with_(Cout=0), INV),
        (with_(ksize=2), UNS), (with_(stride=3), UNS), (with_(stride=2, ksize=1), UNS), (with_(stride=2, upsample=1), UNS),
        (with_(upsample=2, ksize=1), UNS), (with_(Cin=12), UNS), (with_(in_pitch=36), UNS), (with_(in_off=4), UNS),
        (with_(in2=X2, Cin2=4, in2_pitch=32), UNS), (with_(in2=X2, Cin2=16, in2_pitch=36), UNS), (with_(in2=X2, Cin2=0, in2_pitch=32), UNS),
        (with_(out_mode=4), INV), (with_(out_mode=-1), INV),
        (with_(residual=R, res_pitch=40, out_mode=C.PLANAR32), UNS), (with_(residual=R, res_pitch=40, out_mode=C.PLANAR16), UNS),
        (with_(in_off=24), INV), (with_(out_off=16), INV), (with_(in_off=-8), INV), (with_(out_off=-8), INV),
        (with_(in2=X2, Cin2=16, in2_pitch=32, in2_off=24), INV), (with_(in2=X2, Cin2=16, in2_pitch=32, in2_off=-8), INV),
        (with_(residual=R, res_pitch=40, res_off=16), INV), (with_(residual=R, res_pitch=24, res_off=0), INV),
        (with_(residual=R, res_pitch=40, res_off=-8), INV),
        (with_(out_mode=C.PLANAR16, plane_pitch=15), INV), (with_(cout_tile=48), INV), (with_(cout_tile=64, upsample=2), INV),
        (with_(Cin=8, in2=X2, Cin2=16, in2_pitch=32), UNS),          # a stage would straddle the two sources
        (with_(k_wrap=1, Cin=8), UNS), (with_(k_wrap=1, upsample=1), UNS),
        (with_(groups=2, residual=R, res_pitch=40), UNS), (with_(groups=2, upsample=2), UNS),
        (with_(groups=2, group_in_step=4, group_out_step=0), INV), (with_(groups=2, group_in_step=8, group_out_step=-8), INV),
        (with_(groups=2, group_in_step=8, group_out_step=8), INV),          # 8 + 8 + 32 > 40
        (with_(gn_coef=coef.data_ptr(), in_off=0, stride=2), UNS), (with_(gn_coef=coef.data_ptr(), in_off=8), UNS),
        (with_(gn_coef=coef.data_ptr(), in_off=0, out_lo=LO), UNS),
        (with_(gn_coef=coef.data_ptr(), in_off=0), UNS),          # the 32-wide tile has no GroupNorm-prologue instantiation
        (with_(residual_lo=R), INV), (with_(residual=R, res_pitch=40, residual_lo=R), INV),
        (with_(out_lo=LO, out_off=4, out_pitch=36), UNS), (with_(out_lo=LO, upsample=1), UNS),
        (with_(out_lo=LO), UNS),          # a 3x3 pair output exists for the 128-wide tile only
    ]
    for i, (d, want) in enumerate(table):
        assert lib.glare_conv2d_bf16(ctypes.byref(d), ops.stream_handle()) == want, "row %d" % i
    torch.cuda.synchronize()
    H.assert_same_bits(out.flat, out._sentinel(out.flat.numel()), "a refused conv wrote to its output")
    H.assert_same_bits(lo.flat, lo._sentinel(lo.flat.numel()), "a refused conv wrote to its lo output")
    # ... and the same descriptor, valid: every output element 9 x 16 ones on the interior
    assert lib.glare_conv2d_bf16(ctypes.byref(base()), ops.stream_handle()) == 0
    assert float(out.view[0, 1, 1, 8]) == 144.0 and float(out.view[1, 0, 0, 39]) == 64.0


def test_smallcin_and_ws_refuse_before_any_launch(prec):
    dt = ops.act_dtype()
    lib = _lib.lib()
    x = torch.ones(2 * 5 * 4 * 4, device="cuda")
    w = torch.ones(8 * 5 * 9, device="cuda")
    out, lo = _Out((2, 4, 4, 16), False), _Out((2, 4, 4, 16), False)
    s = ops.stream_handle()
    P = _lib.ptr

    def small(cin=3, cout=8, k=3, pitch=16, off=8, f32=0, Bn=2):
        return lib.glare_conv2d_smallcin_f32(P(x), cin * 16, 16, 4, 1, P(w), None, P(out.view), Bn, 4, 4, cin, cout, k, pitch, off, 0, f32, s)
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    assert small(cin=5) == UNS and small(cin=0) == UNS and small(k=2) == UNS and small(off=12) == INV and small(Bn=0) == INV and small(cout=0) == INV

    def pair(cout=8, pitch=16, off=8, lo_ptr=P(lo.view)):
        return lib.glare_conv2d_smallcin_hilo_f32(P(x), 48, 16, 4, 1, P(w), None, P(out.view), lo_ptr, 2, 4, 4, 3, cout, 3, pitch, off, 0, s)
    assert pair(cout=6) == UNS and pair(pitch=12, off=4) == UNS and pair(lo_ptr=None) == INV
    xa = torch.ones(1, 2, 2, 144, dtype=dt, device="cuda")
    wa = torch.ones(128, 128, dtype=dt, device="cuda")
    oa = _Out((1, 2, 2, 136), False)

    def ws(cin=128, cout=128, xp=144, xo=8, op=136, oo=8, r=None, rp=0, ro=0, Bn=1):
        return lib.glare_conv1x1_ws_bf16(P(xa), xp, xo, P(wa), None, r, rp, ro, P(oa.view), op, oo, Bn, 4, cin, cout, 0, None, s)
    assert ws(cin=64) == UNS and ws(cout=64) == UNS and ws(xo=4) == UNS and ws(xo=24) == UNS and ws(oo=16) == UNS and ws(op=132, oo=4) == UNS
    assert ws(r=P(xa), rp=144, ro=24) == UNS and ws(r=P(xa), rp=140, ro=0) == UNS and ws(Bn=0) == INV
    assert lib.glare_conv1x1_ws_image_bf16(P(xa), 144, 8, P(wa), 0, None, 0, None, 0, 0, P(oa.view), 136, 8, 1, 4, 128, 128, 0, None, s) == INV
    torch.cuda.synchronize()
    for o in (out, lo, oa):
        H.assert_same_bits(o.flat, o._sentinel(o.flat.numel()), "a refused launch wrote to its output")
