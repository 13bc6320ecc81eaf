"""CPU: the restatements of tests/conv_fp64.py against F.conv2d, F.interpolate and F.pad in fp64 on EVERY geometry that
test_gpu_conv_edges.py launches, the data-gradient form against fp64 autograd, the sub-pixel form against the plain upsample form on
unrounded filters -- and the SENSITIVITY of what the GPU file compares with, on its own operand generators: the expected bits of the
EQUAL checks change, and the ratio of the BOUNDED checks exceeds 1, when one tap product is removed, one halo column is shifted by one,
row H of an image is read from row 0 of the next image, the bias of channel co + 1 is used, or the K tail is dropped.  The integer
operands are checked for what makes them worth running: every exact result (and every magnitude sum, so every partial sum of every
order) representable in the output format, and no operand tensor zero in half of its elements."""
import pytest
import torch
import torch.nn.functional as F

import conv_fp64 as C

REL = 1e-12
FORMATS = (torch.bfloat16, torch.float16)
IDS = [c["name"] for c in C.IGEMM_CASES]


def _close(got, want, what, rel=REL):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(want.abs().max())
    assert scale > 0, what
    assert float((got - want).abs().max()) / scale < rel, what


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _torch_conv(x_nhwc, w, stride, upsample):
    x = _nchw(x_nhwc)
    if upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, None, 2, 0) if stride == 2 else F.conv2d(x, w, None, 1, w.shape[2] // 2)
    return y.permute(0, 2, 3, 1)


# ---- the restatement is the operator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.IGEMM_CASES, ids=IDS)
def test_restatement_equals_torch_on_every_gpu_geometry(c):
    o = C.case_operands(c, "normal", torch.float16)
    x = o["x"] if o["x2"] is None else torch.cat([o["x"], o["x2"]], -1)
    want = _torch_conv(x, o["w"], c["stride"], c["ups"])
    assert tuple(want.shape[1:3]) == C.out_size(c["H"], c["W"], c["k"], c["stride"], c["ups"])
    _close(C.conv_acc(x, o["w"], c["stride"], c["ups"]), want, c["name"])
    if c["subpixel"]:          # the four phase filters of the unrounded taps give the same operator
        _close(C.subpixel_conv(x, C.subpixel_filters(o["w"])), want, c["name"] + " sub-pixel")
    # through whole buffers: windows at offsets of NaN-filled buffers, the second source, bias, residual
    lay = C.case_layout(c)
    xb = torch.full((c["B"], c["H"], c["W"], lay["in_pitch"]), float("nan"), dtype=torch.float64)
    xb[..., lay["in_off"]:lay["in_off"] + c["cin"]] = o["x"]
    x2b = None
    if c["cin2"]:
        x2b = torch.full((c["B"], c["H"], c["W"], lay["in2_pitch"]), float("nan"), dtype=torch.float64)
        x2b[..., lay["in2_off"]:lay["in2_off"] + c["cin2"]] = o["x2"]
    rb = None
    if c["res"]:
        rb = torch.full(tuple(want.shape[:3]) + (lay["res_pitch"],), float("nan"), dtype=torch.float64)
        rb[..., lay["res_off"]:lay["res_off"] + c["cout"]] = o["res"]
    ref = C.conv_front(xb, o["w"], o["bias"], cin=c["cin"], in_off=lay["in_off"], x2_buf=x2b, cin2=c["cin2"] or None, in2_off=lay["in2_off"],
                       stride=c["stride"], upsample=c["ups"], residual_buf=rb, res_off=lay["res_off"])
    full = want + (o["bias"] if c["bias"] else 0.0) + (o["res"] if c["res"] else 0.0)
    _close(ref.pre(), full, c["name"] + " front end")
    _close(ref.mag, _torch_conv(x.abs(), o["w"].abs(), c["stride"], c["ups"]), c["name"] + " magnitudes")
    one = C.case_reference(c, o)
    if not c["subpixel"]:
        assert torch.equal(one.pre(), ref.pre()) and torch.equal(one.mag, ref.mag)
    acts = {"none": lambda t: t, "relu": torch.relu, "sigmoid": torch.sigmoid, "swish": F.silu}
    assert torch.allclose(ref.value(c["act"]), acts[c["act"]](full), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("c", C.IGEMM_CASES, ids=IDS)
def test_dispatch_restated_for_every_case(c):
    assert C.case_dispatch(c) == c["want"], (c["name"], C.case_dispatch(c))
    lay = C.case_layout(c)
    assert lay["in_pitch"] > lay["in_off"] + c["cin"] and lay["in_off"] % 8 == 0 and lay["in_pitch"] % 8 == 0
    assert c["cin2"] == 0 or c["cin"] % C.pick_tile(c["k"], c["cout"])[1] == 0          # the split lies on a stage boundary
    assert not C.ws_supported(c["cin"], c["cout"]) or c["mode"] != C.NHWC16 or c["k"] == 3


def test_every_igemm_family_has_a_case():
    have = {(c["want"][0], c["want"][2]) for c in C.IGEMM_CASES}
    assert {("k3s1", "fast"), ("k3s1", "planar"), ("k3s1", "general"), ("k3s2", "fast"), ("k3s2", "general"), ("k1", "fast"), ("k1", "general"),
            ("k2", "fast")} <= have
    assert {c["want"][1] for c in C.IGEMM_CASES} == {128, 64, 32}
    # tile edges: sides below, at and above the 8 x 32 tile and its multiples; K stages: whole, with a tail, several
    assert {1, 7, 8, 9, 17} <= {c["H"] for c in C.IGEMM_CASES} and {1, 31, 32, 33, 65} <= {c["W"] for c in C.IGEMM_CASES}
    assert {8, 16, 24, 32, 40, 72, 128} <= {c["cin"] for c in C.IGEMM_CASES}
    assert {3, 8, 32, 40, 64, 72, 128, 136, 256} <= {c["cout"] for c in C.IGEMM_CASES}


# ---- the integer operands: representable, exact in every order, dense -----------------------------------------------------------------
@pytest.mark.parametrize("c", C.IGEMM_CASES, ids=IDS)
def test_integer_operands_are_exact_and_dense(c):
    o = C.case_operands(c, "int", None)
    ref = C.case_reference(c, o, torch.bfloat16)
    limit = C.LIMIT[torch.float32] if c["mode"] in (C.NHWC32, C.PLANAR32) else C.LIMIT[torch.bfloat16]          # bf16: the narrower format
    for t in (ref.acc + ref.bias, ref.pre()):
        assert float(t.abs().max()) <= limit, (c["name"], float(t.abs().max()))
    assert float(ref.mag_all().max()) <= 2.0 ** 24          # every partial sum of every accumulation order is an exact fp32 integer
    assert torch.equal(ref.pre(), ref.pre().round())
    for dtype in FORMATS:
        if c["act"] in ("none", "relu"):
            assert torch.equal(C.staged16(ref, c["act"], dtype), ref.value(c["act"]))          # the two roundings round nothing here
    for name in ("x", "x2", "w", "res"):
        if o[name] is not None:
            assert float((o[name] == 0).double().mean()) < 0.5, (c["name"], name)
    # a removed product is visible in more than half of the elements it belongs to: |x w| = 0 there for less than half of them
    x = o["x"] if o["x2"] is None else torch.cat([o["x"], o["x2"]], -1)
    co, ci = 0, x.shape[-1] - 1
    tap = int(o["w"][co, ci].abs().flatten().argmax())
    assert float(o["w"][co, ci].flatten()[tap]) != 0 and float((x[..., ci] == 0).double().mean()) < 0.5


def test_ternary_sum_magnitude_at_k_1152():
    """the arithmetic behind int_density: +-1 activations against +-1 taps at density 0.54, K = 1152 -> sums of about 25 rms"""
    c = next(c for c in C.IGEMM_CASES if c["cin"] == 128 and c["k"] == 3)
    ref = C.case_reference(c, C.case_operands(c, "int", None))
    rms = float(ref.acc.pow(2).mean().sqrt())
    assert 20.0 < rms < 30.0 and float(ref.pre().abs().max()) < 2.0 ** 8, rms


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------------
FAULTS = ("tap", "halo column", "next image row", "bias", "K tail")
SENSITIVE = ("k3s1 128 ragged", "k3s1 136 K=1152", "k3s2 64 even res", "k3s1 32 upsample", "k1 72 K tail")


def _faulty(c, o, fault):
    """the restatement with one fault injected -> acc, or None where the case has no such element (a 1x1 has no halo, B = 1 no next image,
    an odd side under stride 2 never reads its far padding)"""
    x = o["x"] if o["x2"] is None else torch.cat([o["x"], o["x2"]], -1)
    w, bias = o["w"].clone(), o["bias"]
    xp = C.padded_input(x, c["ups"])
    IH, IW = xp.shape[1] - 2, xp.shape[2] - 2
    OH, OW = C.out_size(c["H"], c["W"], c["k"], c["stride"], c["ups"])
    if fault == "tap":
        ci = x.shape[-1] - 1
        w[0, ci].view(-1)[int(w[0, ci].abs().flatten().argmax())] = 0.0
    elif fault == "halo column":
        if c["k"] == 1 or (c["stride"] == 2 and IW % 2):
            return None, None
        if c["stride"] == 1:
            xp[:, :, 0] = xp[:, :, 1]
        else:
            xp[:, :, IW + 1] = xp[:, :, IW]
    elif fault == "next image row":
        if c["k"] == 1 or c["B"] < 2 or (c["stride"] == 2 and IH % 2):
            return None, None
        xp[:-1, IH + 1] = xp[1:, 1]
    elif fault == "bias":
        bias = bias.roll(-1)
    elif fault == "K tail":
        kc = C.pick_tile(c["k"], c["cout"])[1]
        if x.shape[-1] % kc == 0:
            return None, None
        w[:, x.shape[-1] // kc * kc:] = 0.0
    return C.conv_taps(xp, w, c["stride"], OH, OW), bias


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("name", SENSITIVE)
def test_comparisons_see_an_injected_fault(name, fault):
    c = next(c for c in C.IGEMM_CASES if c["name"] == name)
    seen = 0
    for dtype in FORMATS:
        for family in ("int", "normal"):
            o = C.case_operands(c, family, dtype)
            ref = C.case_reference(c, o, dtype)
            acc, bias = _faulty(c, o, fault)
            if acc is None:
                continue
            assert torch.equal(_faulty(c, o, None)[0], ref.acc)          # without a fault the same code path is the restatement
            bad = C.Ref(acc, ref.mag, bias, ref.res, ref.has_res)
            if family == "int":
                a, b = C.staged16(ref, c["act"], dtype).to(dtype), C.staged16(bad, c["act"], dtype).to(dtype)
                differ = a.view(torch.int16) != b.view(torch.int16)
                assert bool(differ.any()), (name, fault, "EQUAL does not see it")
                if fault == "tap" and c["act"] == "none":
                    assert float(differ[..., 0].double().mean()) > 0.5
                assert bool((ref.value(c["act"]).float() != bad.value(c["act"]).float()).any())          # fp32 outputs alike
            else:
                exact, slack = C.case_bound(c, ref, dtype)
                ratio = (bad.value(c["act"]) - exact).abs() / (0.5 * C.ulp16(exact, dtype) + slack + C.binade_extra(exact, slack, dtype))
                assert float(ratio.max()) > 1.0, (name, fault, float(ratio.max()))
            seen += 1
    assert seen or (fault, name) in {("halo column", "k1 72 K tail"), ("next image row", "k1 72 K tail"), ("next image row", "k3s1 136 K=1152"),
                                     ("K tail", "k3s1 136 K=1152"), ("K tail", "k3s1 32 upsample")}, (name, fault)


def test_every_fault_is_seen_by_some_case():
    for fault in FAULTS:
        assert any(_faulty(c, C.case_operands(c, "int", None), fault)[0] is not None
                   for c in C.IGEMM_CASES if c["name"] in SENSITIVE), fault


# ---- the other restatements ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 3))
def test_dgrad_filter_is_the_input_gradient(k):
    g = torch.Generator().manual_seed(k)
    B, Ci, Co, H, W, P = 2, 5, 6, 7, 9, 8
    x = torch.randn(B, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64)
    gy = torch.randn(B, Co, H, W, generator=g, dtype=torch.float64)
    F.conv2d(x, w, None, 1, k // 2).backward(gy)
    gpad = torch.cat([gy.permute(0, 2, 3, 1), torch.zeros(B, H, W, P - Co, dtype=torch.float64)], -1)
    got = C.conv_acc(gpad, C.dgrad_filter(w, P))
    _close(got, x.grad.permute(0, 2, 3, 1), "dgrad k%d" % k)
    assert float(C.dgrad_filter(w, P)[:, Co:].abs().max()) == 0.0


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("k,cin", ((1, 1), (3, 3), (3, 4), (1, 4)))
def test_smallcin_equals_torch_through_strides(k, cin, layout):
    g = torch.Generator().manual_seed(k * 10 + cin)
    B, H, W, Co = 2, 3, 5, 7
    x = torch.randn(B, H, W, cin, generator=g, dtype=torch.float64)
    w, b = torch.randn(Co, cin, k, k, generator=g, dtype=torch.float64), torch.randn(Co, generator=g, dtype=torch.float64)
    if layout == "nchw":
        flat, strides = x.permute(0, 3, 1, 2).contiguous().reshape(-1), (cin * H * W, H * W, W, 1)
    else:          # channels inside a wider record
        rec = torch.full((B, H, W, cin + 2), float("nan"), dtype=torch.float64)
        rec[..., 1:1 + cin] = x
        flat, strides = rec.reshape(-1)[1:], (H * W * (cin + 2), 1, W * (cin + 2), cin + 2)
    ref = C.smallcin(flat, strides, B, H, W, w, b)
    _close(ref.pre(), _torch_conv(x, w, 1, False) + b, "smallcin")


def test_split3_drops_exactly_the_lo_lo_term():
    g = torch.Generator().manual_seed(3)
    for dtype in FORMATS:
        x = torch.randn(1, 5, 6, 16, generator=g)
        w = torch.randn(8, 16, 3, 3, generator=g) * 0.1
        x_hi = x.to(dtype).double()
        x_lo = (x - x_hi.float()).to(dtype).double()
        acc, mag, dropped = C.split3(x_hi, x_lo, w.double(), dtype)
        w_hi = w.to(dtype).double()
        w_lo = (w - w_hi.float()).to(dtype).double()
        full = C.conv_acc(x_hi + x_lo, w_hi + w_lo)
        assert float((full - acc).abs().max()) > 0 and bool(((full - acc).abs() <= dropped * (1 + 1e-9)).all())
        _close(acc + C.conv_acc(x_lo, w_lo), full, "split3")
        assert bool((mag >= acc.abs() * (1 - 1e-12)).all())


def test_feedback_round_keeps_the_channel_sum():
    g = torch.Generator().manual_seed(4)
    w = torch.randn(6, 40, generator=g) * 0.05
    for dtype in FORMATS:
        q = C.feedback_round(w, dtype)
        assert torch.equal(q.to(dtype).double(), q)
        half_ulp = 0.5 * C.ulp16(w.abs().max(1).values.double(), dtype)
        assert bool(((q - w.double()).sum(1).abs() <= half_ulp * 1.0001).all())


def test_gn_stats_layout_and_pair16():
    g = torch.Generator().manual_seed(5)
    y = torch.randn(2, 3, 4, 128, generator=g, dtype=torch.float64)
    s, m = C.gn_stats(y)
    assert tuple(s.shape) == (2, 1, 32, 2)
    _close(s[1, 0, 5, 0].reshape(1), y[1, :, :, 20:24].sum().reshape(1), "sum")
    _close(s[0, 0, 31, 1].reshape(1), (y[0, :, :, 124:] ** 2).sum().reshape(1), "sum of squares")
    assert bool((m[..., 0] >= s[..., 0].abs()).all())
    for dtype in FORMATS:
        hi, lo = C.pair16(y, dtype)
        assert bool(((hi.double() + lo.double() - y).abs() <= C.pair_slack(y, 0.0, dtype)).all())          # 2^-22-class in fp16, 2^-16 in bf16


def test_place_and_owned_are_inverse():
    vals = torch.arange(2 * 3 * 4 * 5, dtype=torch.float64).reshape(2, 3, 4, 5)
    nhwc = torch.full((2, 3, 4, 9), -1.0)
    e = C.place(nhwc, vals, C.NHWC32, 2)
    assert torch.equal(C.owned(e, vals.shape, C.NHWC32, 2).double(), vals) and float(e[..., :2].max()) == -1.0 and float(e[..., 7:].max()) == -1.0
    planes = torch.full((2, 8, 16), -1.0)
    e = C.place(planes, vals, C.PLANAR32, 1)
    assert torch.equal(C.owned(e, vals.shape, C.PLANAR32, 1).double(), vals)
    assert float(e[:, 1:6, 12:].max()) == -1.0 and float(e[:, 0].max()) == -1.0 and float(e[:, 6:].max()) == -1.0
    assert float(e[1, 3, 1 * 4 + 2]) == float(vals[1, 1, 2, 2])          # plane co, pixel oy OW + ox


def test_bound_helpers():
    for dtype in FORMATS:
        m, emin = C.fmt(dtype)
        v = torch.tensor([1.0, 1.5, 2.0, 2.0 ** emin, 2.0 ** (emin - 3), 0.0], dtype=torch.float64)
        want = torch.tensor([2.0 ** -m, 2.0 ** -m, 2.0 ** (1 - m), 2.0 ** (emin - m), 2.0 ** (emin - m), 2.0 ** (emin - m)], dtype=torch.float64)
        assert torch.equal(C.ulp16(v, dtype), want)
        x = torch.tensor([2.0 - 2.0 ** -20], dtype=torch.float64)
        assert float(C.binade_extra(x, torch.tensor([2.0 ** -19], dtype=torch.float64), dtype)) == 0.5 * 2.0 ** -m
        assert float(C.binade_extra(torch.tensor([1.5], dtype=torch.float64), torch.tensor([2.0 ** -19], dtype=torch.float64), dtype)) == 0.0
    assert C.padded_k(3, 24) == 288 and C.padded_k(1, 40) == 64 and C.padded_k(3, 24, subpixel=True) == 128
    assert C.ws_supported(128, 1024) and not C.ws_supported(128, 1536) and not C.ws_supported(64, 128) and C.ws_supported(256, 64, split=True)
