"""GPU: the kernels every printed PSNR, SSIM and LPIPS rests on -- csrc/harness.hip (pre_kernel, pre_pad_kernel, post_crop / post_gain / post_psnr
/ post_count, to_ubyte, ubyte_planes, post_u8 / post_u8_count, gain_partial / gain_final, score_u8 / score_final) and csrc/metrics.hip
(conv_direct_f32, maxpool_f32, lpips_tap / lpips_finish) -- PER ELEMENT against the fp64 restatements of tests/scoring_fp64.py (held to
independent references and shown sensitive on the CPU: test_vq_scoring_fp64_host.py), at the shapes where their index arithmetic changes
regime: the second block of the one-thread-per-image finish kernels (B = 65), the second trip of the word and pixel loops (131 949 bytes,
43 983 and 16 512 pixels per image), words that straddle two images, pads folded many times over a 2-pixel side, the ragged output-channel
group, block and input-channel chunk of the convolution, the pool's grid-stride loop beyond 65 535 blocks.

Where a result has no rounding of its own (an index map, a clamp, a byte, an integer sum, a maximum) the test asserts bit equality; every
other bound is counted from the kernel's expression next to the restatement that returns it (scoring_fp64.py) or next to the call here, and
goes through tolerances.within(measured / bound, 1.0, tag)."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_fp64
import scoring_fp64 as S
from fp64_bounds import U, _tag, assert_f32
from glare_amd import _lib, harness, metrics
from glare_amd._lib import ptr, stream_handle
from test_gpu_loss_update_edges import TINY, V, _moment_bounds
from tolerances import within

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _np(t):
    return t.detach().cpu().numpy()


def _bits_equal(got, want):
    return np.array_equal(S.bits32(_np(got) if torch.is_tensor(got) else got), S.bits32(want))


# ---- B. paired harness: the value of a byte, then pure indexing -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table32():
    """the 256 values the three pre-processing kernels can produce, from a 1 x 256 ramp through pre_pad_kernel without padding: checked against
    fp64 once, to the limit test_gpu_harness.py asserts (3e-7 relative + 3e-7 absolute: one ulp of logf); everything after is bit equality"""
    ramp = torch.arange(256, dtype=torch.uint8).view(1, 1, 256, 1).expand(1, 1, 256, 3).contiguous().cuda()
    out = _np(harness.preprocess_unpaired_device(ramp, (0, 0, 0, 0), harness.PAD_REFLECT101))
    assert out.shape == (1, 3, 1, 256) and out.dtype == np.float32
    assert np.array_equal(S.bits32(out[0, 0]), S.bits32(out[0, 1])) and np.array_equal(S.bits32(out[0, 0]), S.bits32(out[0, 2]))
    t64 = S.pre_table64()
    within(float((np.abs(out[0, 0, 0].astype(np.float64) - t64) / (3e-7 * np.abs(t64) + 3e-7)).max()), 1.0, "pre:table")
    return out[0, 0, 0].copy()


@pytest.mark.parametrize("shape", S.PAIRED_SHAPES, ids=["%dx%dx%d" % s for s in S.PAIRED_SHAPES])
def test_paired_preprocess_is_the_table_at_np_pads_indices(table32, shape):
    """(2,2,2): period 2, folded ten times; (1,21,20) / (1,20,21): a side equal to the pad; (2,3,40): a 3-pixel side under a 20-pixel pad"""
    B, H, W = shape
    img = np.random.RandomState(H * 100 + W).randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    got = harness.preprocess_device(torch.from_numpy(img).cuda())
    want = S.pre_expected(table32, img, S.pad_indices(H, 0, S.PAD, "reflect"), S.pad_indices(W, S.PAD, 0, "reflect"))
    assert tuple(got.shape) == want.shape == (B, 3, H + S.PAD, W + S.PAD)
    assert _bits_equal(got, want)


@pytest.mark.parametrize("mode", ("reflect", "symmetric"))
@pytest.mark.parametrize("case", S.PAD_CASES, ids=["%dx%d:%d.%d.%d.%d" % ((c[0], c[1]) + c[2]) for c in S.PAD_CASES])
def test_pad_preprocess_is_the_table_at_np_pads_indices(table32, case, mode):
    H, W, (t, b, l, r) = case
    img = np.random.RandomState(H * 10 + W + t).randint(0, 256, size=(2, H, W, 3)).astype(np.uint8)
    flag = harness.PAD_REFLECT101 if mode == "reflect" else harness.PAD_SYMMETRIC
    got = harness.preprocess_unpaired_device(torch.from_numpy(img).cuda(), (t, b, l, r), flag)
    want = S.pre_expected(table32, img, S.pad_indices(H, t, b, mode), S.pad_indices(W, l, r, mode))
    assert tuple(got.shape) == want.shape == (2, 3, H + t + b, W + l + r)
    assert _bits_equal(got, want)


def _post(out, gt, h, w):
    o = torch.from_numpy(out).cuda()
    g = None if gt is None else torch.from_numpy(gt).cuda()
    return harness.postprocess_device(o, h, w, g, want_nonfinite=True)


@pytest.mark.parametrize("shape", S.POST_SHAPES, ids=["%dx%dx%d" % s for s in S.POST_SHAPES])
def test_postprocess_with_ground_truth_per_element(shape):
    """B = 65 at 5 x 7: the finish kernels' second block; 127 x 129 / 128 x 128 / 129 x 128: one pixel short of a trip of the 64 x 256 pixel
    loops, exactly one, and a ragged second.  The tensor is larger than the crop below it and to its right."""
    B, h, w = shape
    out, gt = S.post_inputs(B, h, w, seed=h * 1000 + w)
    ref = S.post_fp64(out, gt, h, w)
    restored, ps, bad = _post(out, gt, h, w)
    restored2, ps2, _ = _post(out, gt, h, w)
    tag = "post:%dx%dx%d" % shape
    assert tuple(restored.shape) == (B, h, w, 3) and ps.dtype == torch.float64 and bad.dtype == torch.int32
    # scoring_fp64.post_fp64: 3 roundings of gray(r), (float) gain, r * gain -> gamma(5) |r gain|
    assert_f32(restored.cpu(), torch.from_numpy(ref["restored"]), torch.from_numpy(ref["bound"]), tag + ":restored")
    within(float((np.abs(_np(ps) - ref["psnr"]) / ref["psnr_bound"]).max()), 1.0, _tag(tag + ":psnr"))
    assert _np(bad).tolist() == [0] * B
    assert torch.equal(restored.view(torch.int32), restored2.view(torch.int32)) and torch.equal(ps.view(torch.int64), ps2.view(torch.int64))
    # without ground truth: the crop and the clamp, no rounding at all
    plain, none, bad0 = _post(out, None, h, w)
    assert none is None and _bits_equal(plain, ref["crop"]) and _np(bad0).tolist() == [0] * B


def test_postprocess_nonfinite_values_stay_in_their_image():
    B, h, w = S.POST_SHAPES[0]
    out, gt = S.post_inputs(B, h, w, seed=1)
    inside = {0: ("nan", "+inf"), 63: ("nan", "-inf"), 64: ("nan", "+inf", "-inf")}
    spec = S.plant_specials(out, h, w, inside, (1, 30, 62))
    clean_r, clean_p, clean_bad = _post(out, gt, h, w)
    restored, ps, bad = _post(spec, gt, h, w)
    assert _np(clean_bad).tolist() == [0] * B
    assert _np(bad).tolist() == S.post_fp64(spec, gt, h, w)["nonfinite"].tolist() == [2] + [0] * 62 + [2, 3]
    for b in range(B):
        if b in inside:          # a NaN stays a NaN in restored (the gain of its image is NaN with it), so the PSNR is NaN
            assert bool(torch.isnan(restored[b]).all()) and bool(torch.isnan(ps[b])), b
        else:
            assert torch.equal(restored[b].view(torch.int32), clean_r[b].view(torch.int32)), b
            assert torch.equal(ps[b].view(torch.int64), clean_p[b].view(torch.int64)), b
    plain, _, bad0 = _post(spec, None, h, w)
    crop, cnt = S.post_crop(spec, h, w)
    assert _bits_equal(plain, crop) and _np(bad0).tolist() == cnt.tolist()


@pytest.mark.parametrize("n", S.UBYTE_N)
def test_to_ubyte_and_the_x255_plane_round_ties_to_even(n):
    x = S.ubyte_inputs(n)
    want = S.to_ubyte_expected(x)
    xd = torch.from_numpy(x).cuda()
    assert np.array_equal(_np(harness.to_ubyte_device(xd)), want.astype(np.uint8))
    gt = torch.from_numpy(np.random.RandomState(n).randint(0, 256, size=n).astype(np.uint8)).cuda()
    x255 = torch.full((n + 32,), -7.0, dtype=torch.float32, device="cuda")
    y255 = torch.full((n + 32,), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().glare_harness_ubyte_planes_f32(ptr(xd), ptr(gt), n, ptr(x255), ptr(y255), stream_handle()), "glare_harness_ubyte_planes_f32")
    assert bool((x255[:n].double().cpu() == torch.from_numpy(want)).all())          # as numbers: -0.0 * 255 may keep its sign
    assert torch.equal(y255[:n], gt.float()) and bool((x255[n:] == -7.0).all()) and bool((y255[n:] == -7.0).all())


# ---- the evaluation loop's SSIM --------------------------------------------------------------------------------------------------------------
_cond_rows = {}
COND_HEADER = """
SSIM of the evaluation loop (glare_amd.harness.ssim_device: rint(clip * 255) planes, C1 = 6.5025, C2 = 58.5225), measured on an MI355X.
Written by tests/test_gpu_scoring_edges.py::test_ssim_metric_per_image at B 2, 12 x 27, C 3, the 11-tap window; `error` the largest
|value - fp64| over the images, `bound` the largest bound the test derives (the moments' fma chains and U (E[xx] + mu^2) of the variance's
cancellation over v2 >= C2 = 58.5225, through loss_fp64 / test_gpu_loss_update_edges's counting).

family            error       bound    U (E[xx] + mu^2) / C2
"""


def _metric_bound(x, y, mom):
    """ssim_fwd_kernel's expression on the stored moments, in its order, on V operands with the metric's constants -> (exact mean, bound)"""
    w1 = S.metric_window()
    bmom = _moment_bounds(x, y, w1)
    m1, m2, e11, e22, e12 = (V(mom[..., k], bmom[..., k]) for k in range(5))
    s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
    v1, v2 = s12.scale(2.0) + S.METRIC_C2, (s1 + s2) + S.METRIC_C2
    a1, a2 = m1.scale(2.0) * m2 + S.METRIC_C1, (m1 * m1 + m2 * m2) + S.METRIC_C1
    ss = (a1 * v1) / (a2 * v2)
    est = U * float((mom[..., 2] + mom[..., 0] ** 2).max()) / S.METRIC_C2
    return ss.v.mean(), ss.e.mean() + U * ss.v.mean().abs() + 1e-13, est          # block sums in double; one rounding to float


@pytest.mark.parametrize("family", S.SSIM_FAMILIES)
@pytest.mark.parametrize("shape", S.SSIM_SHAPES, ids=["%dx%dx%d" % s for s in S.SSIM_SHAPES])
def test_ssim_metric_per_image(shape, family):
    """(3,11,11): one valid position per channel; (2,12,27): ragged; (1,40,23): taller than wide.  The reference is the fp64 SSIM of the
    ROUNDED planes (scoring_fp64.to_ubyte_expected), so the rounding of the restored image to uint8 is inside the comparison."""
    res32, gt = S.ssim_inputs(shape, family, sum(shape))
    got = harness.ssim_device(torch.from_numpy(res32).cuda(), torch.from_numpy(gt).cuda())
    assert got.dtype == torch.float64 and tuple(got.shape) == (shape[0],)
    x = torch.from_numpy(S.to_ubyte_expected(res32)).cuda()
    y = torch.from_numpy(gt.astype(np.float64)).cuda()
    worst = (0.0, 0.0, 0.0)
    for b in range(shape[0]):
        mom, esim, _ = loss_fp64.ssim_forward(x[b:b + 1], y[b:b + 1], S.metric_window(), S.METRIC_C1, S.METRIC_C2)
        mean, bound, est = _metric_bound(x[b:b + 1], y[b:b + 1], mom)
        assert abs(float(mean - esim)) < 1e-11
        err = abs(float(got[b]) - float(esim))
        within(err / float(bound), 1.0, "ssim_metric:%dx%dx%d:%s" % (shape + (family,)))
        if family == "identical":
            within(abs(float(got[b]) - 1.0) / float(bound), 1.0, "ssim_metric:%dx%dx%d:identical_is_1" % shape)
        worst = max(worst, (err, float(bound), est))
    if shape == (2, 12, 27):
        _cond_rows[family] = "%-12s %10.3e  %10.3e  %10.3e\n" % ((family,) + worst)
        outdir = os.path.join(ROOT, os.environ.get("GLARE_OUT_DIR", "out"))
        try:
            os.makedirs(outdir, exist_ok=True)
            with open(os.path.join(outdir, "ssim_metric_conditioning.txt"), "w") as f:
                f.write(COND_HEADER + "".join(_cond_rows[k] for k in S.SSIM_FAMILIES if k in _cond_rows))
        except OSError as e:       # a read-only tree: the checks above have run, only the table is lost
            warnings.warn("ssim_metric_conditioning.txt not written: %s" % e)


# ---- C. second block and second trip of the unpaired / adjust kernels -------------------------------------------------------------------------
def _unpaired_case(name, special):
    if name == "tiny":
        B, Hp, Wp, window = S.TINY_IMAGES
        x, gt = S.tiny_outputs(special)
    else:
        B, Hp, Wp, window = S.SECOND_TRIP
        x, gt_full = S.output_and_gt(B, Hp, Wp, special)
        gt = gt_full[:, :window[2], :window[3]].contiguous()
    return B, Hp, Wp, window, x, gt


@pytest.mark.parametrize("name", ("tiny", "second_trip"))
def test_word_kernels_bytes_counts_and_sums_bit_for_bit(name):
    """tiny: B = 65 images of 27 bytes -- most start mid-word, every last word spills into the next image, the finish kernels run a second
    block, specials sit in images 0, 63, 64 and in spilled bytes.  second_trip: 131 949 bytes per image, a ragged second trip of the word loops."""
    B, Hp, Wp, window, x, gt = _unpaired_case(name, True)
    top, left, h, w = window
    xd, gd = x.cuda(), gt.cuda()
    pads = (top, Hp - top - h, left, Wp - left - w)
    u8, bad = harness.postprocess_unpaired_device(xd, pads, h, w, want_nonfinite=True)
    want_u8, _ = harness.score_u8(x.numpy(), gt.numpy(), None, window)
    assert np.array_equal(_np(u8), want_u8)
    assert _np(bad).tolist() == S.window_nonfinite(x.numpy(), window).sum(1).tolist()
    assert torch.equal(harness.postprocess_unpaired_device(xd, pads, h, w), u8)          # without the count: no partials, the same bytes
    gains = torch.from_numpy(np.random.RandomState(B).uniform(0.5, 2.0, B).astype(np.float32))
    gains[1 % B] = INF          # 0 * inf = NaN -> 0
    if B > 64:
        gains[63], gains[64] = 0.25, NAN
    for gain in (None, gains):
        got_u8, sse = harness.score_device(xd, gd, None if gain is None else gain.cuda(), window)
        want_u8, want_sse = harness.score_u8(x.numpy(), gt.numpy(), None if gain is None else gain.numpy(), window)
        assert np.array_equal(_np(got_u8), want_u8)
        assert sse.dtype == torch.int64 and _np(sse).tolist() == want_sse.tolist()
        again = harness.score_device(xd, gd, None if gain is None else gain.cuda(), window)
        assert torch.equal(again[0], got_u8) and torch.equal(again[1], sse)


@pytest.mark.parametrize("name", ("tiny", "second_trip"))
def test_gain_kernel_second_block_and_second_trip(name):
    """the existing 1e-6 of test_gpu_evaluate.py (two fp64 sums in different orders, rounded to fp32, are at most an ulp = 6e-8 apart) and
    run-to-run bit equality; second_trip: 43 983 pixels against gain_partial_kernel's trip of 32 768"""
    B, Hp, Wp, window, x, gt = _unpaired_case(name, False)
    x = x + 0.6
    xd, gd = x.cuda(), gt.cuda()
    g1 = harness.adjust_gain_device(xd, gd, window)
    g2 = harness.adjust_gain_device(xd, gd, window)
    want = harness.adjust_gain(x.numpy(), gt.numpy(), window).astype(np.float64)
    assert g1.dtype == torch.float32 and tuple(g1.shape) == (B,)
    within(float(np.abs(_np(g1).astype(np.float64) / want - 1).max()) / 1e-6, 1.0, "adjust_gain:" + name)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    xn = x.clone()          # a NaN in one image's window makes that image's gain NaN and no other's
    b = B - 1
    xn[b, 1, window[0] + window[2] - 1, window[1] + window[3] - 1] = NAN
    gn = harness.adjust_gain_device(xn.cuda(), gd, window)
    assert bool(torch.isnan(gn[b])) and torch.equal(gn[:b].view(torch.int32), g1[:b].view(torch.int32))


# ---- D. LPIPS kernels ---------------------------------------------------------------------------------------------------------------------------
def _conv_case(k, st, pd, cin, ohw, cout, seed, bias=True, relu=True, affine=False, B=2):
    H, W = S.conv_input_size(ohw[0], k, st, pd), S.conv_input_size(ohw[1], k, st, pd)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=g)
    if B > 1 and not affine:
        x[1] = 0          # images do not mix: this one's output is act(bias), exactly
    w = torch.randn(cout, cin, k, k, generator=g) * 0.1
    b = torch.randn(cout, generator=g) if bias else None
    sh = sc = None
    if affine:
        sh, sc = torch.randn(cin, generator=g) * 0.1, torch.rand(cin, generator=g) * 0.2 + 0.4
    got = metrics.conv2d_direct(x.cuda(), w.cuda(), None if b is None else b.cuda(), st, pd, relu,
                                None if sh is None else sh.cuda(), None if sc is None else sc.cuda()).cpu()
    exact, bound = S.conv_fp64(x, w, b, st, pd, relu, sh, sc)
    assert tuple(got.shape) == (B, cout, ohw[0], ohw[1])
    tag = "conv:k%ds%dp%d:cin%d:cout%d:%dx%d:%s%s%s" % (k, st, pd, cin, cout, ohw[0], ohw[1], "b" if bias else "-", "r" if relu else "-", "a" if affine else "-")
    assert_f32(got, exact, bound, tag)
    if B > 1 and not affine:
        want = torch.zeros(cout) if b is None else (torch.relu(b) if relu else b)
        assert bool((got[1] == want.view(-1, 1, 1)).all()), tag + ": the zero image's output is not act(bias)"


@pytest.mark.parametrize("kcase", sorted(set(S.ALEX)), ids=lambda c: "k%ds%dp%d" % c)
def test_conv_direct_alexnet_geometries_per_element(kcase):
    """1, 63 and 65 output pixels (a block is 64) x Cout 1, 7, 33, 40 (a thread's group is 8, a block's 32) at the smallest input that gives
    them -- 7 x 7 for the 11-tap filter, 1 x 1 for the others: H < k, every tap but a few in the padding; the first conv's input affine on
    the 11-tap geometry.  (taps + 2 [+ 2 with the affine]) U sum |w| |x'| + U |bias|: scoring_fp64.conv_fp64 counts it."""
    k, st, pd = kcase
    for ohw in S.CONV_OHW:
        for cout in S.CONV_COUT:
            _conv_case(k, st, pd, 3 if k == 11 else 5, ohw, cout, seed=k * 1000 + cout + ohw[1])
            if k == 11:
                _conv_case(k, st, pd, 3, ohw, cout, seed=k * 1000 + cout + ohw[1] + 1, affine=True)


@pytest.mark.parametrize("ccase", S.CONV_CIN, ids=lambda c: "k%ds%dp%d:cin%d" % c)
def test_conv_direct_ragged_channel_chunks_per_element(ccase):
    """Cin across a ragged last chunk of the filter staging: 29 and 57 over chunks of 28, 64 over 10, 3 over 2, 3 over 1 (k = 16, the largest
    filter the kernel takes); without bias, without ReLU"""
    k, st, pd, cin = ccase
    for cout in S.CONV_COUT:
        _conv_case(k, st, pd, cin, (7, 9), cout, seed=cin * 100 + cout)
    _conv_case(k, st, pd, cin, (5, 13), 7, seed=cin, bias=False)
    _conv_case(k, st, pd, cin, (5, 13), 33, seed=cin + 1, relu=False)
    _conv_case(k, st, pd, cin, (1, 1), 40, seed=cin + 2, bias=False, relu=False)


def test_conv_direct_padding_taps_contribute_exactly_zero_under_the_affine():
    """an image that equals `shift` everywhere: x - shift = 0 at every in-range tap, and a padding tap is 0 (not -shift / scale), so the result
    is the bias, exactly"""
    sh, sc = torch.tensor([-.030, -.088, -.188]), torch.tensor([.458, .448, .450])
    g = torch.Generator().manual_seed(11)
    w, b = torch.randn(40, 3, 11, 11, generator=g) * 0.1, torch.randn(40, generator=g)
    for H, W in ((7, 7), (31, 39)):
        x = sh.view(1, 3, 1, 1).expand(2, 3, H, W).contiguous()
        got = metrics.conv2d_direct(x.cuda(), w.cuda(), b.cuda(), 4, 2, False, sh.cuda(), sc.cuda()).cpu()
        assert bool((got == b.view(1, -1, 1, 1)).all())


def test_conv_direct_refuses_a_17_tap_filter():
    x = torch.randn(1, 2, 20, 20, device="cuda")
    w = torch.randn(3, 2, 17, 17, device="cuda")
    out = torch.full((1, 3, 4, 4), -7.0, device="cuda")
    st = _lib.main_lib().glare_conv2d_direct_f32(ptr(x), ptr(w), None, ptr(out), 1, 2, 20, 20, 3, 17, 1, 0, 1, None, None, stream_handle())
    torch.cuda.synchronize()
    assert st == _lib.ERR_UNSUPPORTED and bool((out == -7.0).all())
    with pytest.raises(_lib.GlareError):
        metrics.conv2d_direct(x, w)


def test_maxpool_bits_small_shapes():
    for kk, st, H, W in ((3, 2, 3, 3), (3, 2, 4, 4), (3, 2, 23, 30), (2, 1, 5, 4)):
        x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H * W))
        x[1] *= 64
        got = metrics.maxpool2d(x.cuda(), kk, st).cpu()
        assert torch.equal(got.view(torch.int32), F.max_pool2d(x, kk, st).view(torch.int32))


def test_maxpool_grid_stride_second_trip():
    """16 842 752 outputs > 65 535 blocks x 256 threads: the loop behind the grid cap takes a second trip"""
    x = torch.randn(1, 257, 257, 257, generator=torch.Generator().manual_seed(257))
    got = metrics.maxpool2d(x.cuda(), 2, 1)
    assert got.numel() == 16842752 > 65535 * 256
    assert torch.equal(got.cpu(), F.max_pool2d(x, 2, 1))


def test_relu_and_pool_keep_a_nan():
    """torch.relu and max_pool2d propagate a NaN; a metric that hid one would print a finite LPIPS for a broken image (harness.hip's clamp says
    the same of PSNR)"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 9, 11, generator=g)
    x[0, 2, 4, 5] = NAN
    w, b = torch.randn(7, 5, 3, 3, generator=g) * 0.1, torch.randn(7, generator=g)
    got = metrics.conv2d_direct(x.cuda(), w.cuda(), b.cuda(), 1, 1, True).cpu()
    want = torch.relu(F.conv2d(x.double(), w.double(), b.double(), 1, 1))
    assert int(torch.isnan(want).sum()) == 7 * 9 and torch.equal(torch.isnan(got), torch.isnan(want))
    exact, bound = S.conv_fp64(torch.nan_to_num(x), w, b, 1, 1, True)
    ok = ~torch.isnan(want)
    within(float(((got.double() - exact).abs() / bound)[ok].max()), 1.0, _tag("conv:nan:others"))
    for pos in ((0, 2, 4, 5), (1, 0, 0, 0), (1, 4, 8, 10)):          # inside, the first element of a window, the last
        x = torch.randn(2, 5, 9, 11, generator=g)
        x[pos] = NAN
        got, want = metrics.maxpool2d(x.cuda(), 3, 2).cpu(), F.max_pool2d(x, 3, 2)
        assert bool(torch.isnan(want).any()) and torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))


def _fma_chain_sum(terms, dim):
    """acc = fma(a_c, b_c, acc) over `dim`, the products a_c b_c given as V (their own product rounding counted, which an fma does not
    have): the terms' errors, and one rounding per link on the sum of magnitudes"""
    n = terms.v.shape[dim]
    return V(terms.v.sum(dim), terms.e.sum(dim) + S.gamma(n) * terms.mag().sum(dim))


def _tap_reference(f0, f1, lin, eps):
    """lpips_tap_kernel in its order on V operands -> (exact [B], bound [B]): n = fma chain of C non-negative squares (C roundings),
    sqrt 1, + eps 1, each quotient 1, the difference 1, its square 1, the fma chain over the channels C (+ 1 per term here), then a block's
    sum -- 6 shuffle levels and (r0 + r1) + (r2 + r3): depth 8 -- in fp32; the sum of the blocks, / HW and the accumulation are fp64"""
    f0, f1, lin = f0.cuda().double(), f1.cuda().double(), lin.cuda().double()
    B, C, HW = f0.shape

    def denom(f):
        n = (f * f).sum(1, keepdim=True)
        return V(n, S.gamma(C) * n).sqrt() + eps

    d = V(f0) / denom(f0) - V(f1) / denom(f1)
    acc = _fma_chain_sum(V(lin.view(1, C, 1).expand(B, C, HW).contiguous()) * (d * d), 1)          # [B, HW]
    exact = acc.v.sum(1) / HW
    bound = (acc.e.sum(1) + S.gamma(8) * acc.mag().sum(1)) / HW + 2.0 ** -50 * exact.abs() + TINY
    return exact, bound


def _tap(f0, f1, lin, dist, accumulate, eps=1e-10, short=0):
    lib = _lib.main_lib()
    B, C, HW = f0.shape
    nws = lib.glare_lpips_tap_workspace_bytes(B, HW)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device="cuda")
    return lib.glare_lpips_tap_f32(ptr(f0), ptr(f1), ptr(lin), B, C, HW, eps, accumulate, ptr(dist), ptr(ws), nws - short, stream_handle())


@pytest.mark.parametrize("C", S.TAP_C)
@pytest.mark.parametrize("HW", S.TAP_HW)
def test_lpips_tap_per_image(HW, C):
    """HW 1, 255, 257, 600: one pixel, a block short of one, a second block of one pixel, three blocks; the second image's features scaled by
    1e-5, where eps decides; pixel 0 all zero in one image, pixel 1 in both (no NaN, the exact contribution); accumulate 0 and 1"""
    f0, f1, lin = S.tap_inputs(2, C, HW, seed=HW * 1000 + C)
    f0[1] *= S.TAP_SMALL
    f1[1] *= S.TAP_SMALL
    f0d, f1d, lind = f0.cuda(), f1.cuda(), lin.cuda()
    exact, bound = _tap_reference(f0, f1, lin, S.LPIPS_EPS)
    ref = S.lpips_tap_fp64(f0, f1, lin)
    assert bool(((exact.cpu() - ref).abs() <= 1e-12 * ref.abs() + 1e-300).all())          # the V expression is the restatement's function
    tag = "lpips_tap:hw%d:c%d" % (HW, C)
    dist = torch.full((2,), NAN, dtype=torch.float64, device="cuda")
    assert _tap(f0d, f1d, lind, dist, 0) == 0
    assert bool(torch.isfinite(dist).all())
    within(float(((dist - exact).abs() / bound).max()), 1.0, _tag(tag))
    prior = torch.tensor([0.375, 1e-3], dtype=torch.float64, device="cuda")
    acc = prior.clone()
    assert _tap(f0d, f1d, lind, acc, 1) == 0
    assert torch.equal(acc, prior + dist)          # the prior value is added in fp64, one rounding: the same bits as this sum
    same = torch.full((2,), NAN, dtype=torch.float64, device="cuda")
    assert _tap(f1d, f1d, lind, same, 0) == 0
    assert same.tolist() == [0.0, 0.0]             # d(x, x) = 0 exactly


def test_lpips_tap_finish_second_block():
    """B = 65 at HW = 5: image 64 is the finish kernel's second block"""
    f0, f1, lin = S.tap_inputs(65, 7, 5, seed=65)
    exact, bound = _tap_reference(f0, f1, lin, S.LPIPS_EPS)
    for accumulate in (0, 1):
        prior = torch.arange(65, dtype=torch.float64, device="cuda") * 0.125
        dist = prior.clone()
        assert _tap(f0.cuda(), f1.cuda(), lin.cuda(), dist, accumulate) == 0
        want = exact + prior if accumulate else exact
        within(float(((dist - want).abs() / (bound + 2.0 ** -53 * want.abs())).max()), 1.0, _tag("lpips_tap:b65:acc%d" % accumulate))
    assert len(set(exact.tolist())) == 65          # every image has its own value: a wrong image would be seen


def test_lpips_tap_refusals_leave_the_output_alone():
    f0, f1, lin = (t.cuda() for t in S.tap_inputs(2, 7, 300, seed=3))
    dist = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    lib = _lib.main_lib()
    nws = lib.glare_lpips_tap_workspace_bytes(2, 300)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    s = stream_handle()
    assert nws == 2 * 2 * 4
    assert lib.glare_lpips_tap_f32(ptr(f0), ptr(f1), ptr(lin), 2, 7, 300, 1e-10, 0, ptr(dist), ptr(ws), nws - 1, s) == _lib.ERR_WORKSPACE
    assert lib.glare_lpips_tap_f32(ptr(f0), ptr(f1), ptr(lin), 2, 7, 300, 1e-10, 0, ptr(dist), None, nws, s) == _lib.ERR_WORKSPACE
    assert lib.glare_lpips_tap_f32(ptr(f0), ptr(f1), ptr(lin), 0, 7, 300, 1e-10, 0, ptr(dist), ptr(ws), nws, s) == _lib.ERR_INVALID
    assert lib.glare_lpips_tap_f32(ptr(f0), ptr(f1), ptr(lin), 2, 0, 300, 1e-10, 0, ptr(dist), ptr(ws), nws, s) == _lib.ERR_INVALID
    assert lib.glare_lpips_tap_f32(ptr(f0), ptr(f1), None, 2, 7, 300, 1e-10, 0, ptr(dist), ptr(ws), nws, s) == _lib.ERR_INVALID
    assert lib.glare_lpips_tap_f32(ptr(f0), ptr(f1), ptr(lin), 2, 7, 0, 1e-10, 0, ptr(dist), ptr(ws), nws, s) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert dist.tolist() == [-7.0, -7.0]
    assert lib.glare_lpips_tap_f32(ptr(f0), ptr(f1), ptr(lin), 2, 7, 300, 1e-10, 0, ptr(dist), ptr(ws), nws, s) == 0
    torch.cuda.synchronize()
    assert bool((dist > 0).all())
