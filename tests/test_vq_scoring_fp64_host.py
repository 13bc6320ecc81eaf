"""CPU: tests/vq_fp64.py and tests/scoring_fp64.py, the references of test_gpu_vq_edges.py and test_gpu_scoring_edges.py.
  1. the restatements against independent references: the pre / post-processing against glare_amd.harness (preprocess, postprocess, psnr)
     and tests/golden/harness.npz; the index maps against np.pad; SSIM against oracle.torch_ref.ssim_utils2 and tests/golden/ssim_metric.npz;
     the LPIPS convolution and tap against oracle.torch_ref.LPIPSAlex in double on seeded weights; the fp64 argmin against the C oracle's
     own distances on the random family; the kernel-shaped fp32 search against the C oracle; the word-owning two-level sums against a plain sum;
  2. the families have the property each claims: the midpoint tokens make the oracle differ from the fp64 argmin for at least a quarter of
     them while the random tokens never do; the oracle stays inside the counted fp64 bound on every family; every duplicated pair lies in
     different ranges for 16, 8 and 4 parts (or in different resident chunks); a family at n tokens is the head of the family at more; the
     token counts sit on both sides of each launch-shape switch; fp32 values whose product with 255 is exactly k + 0.5 exist for both
     parities of k;
  3. sensitivity: every named mutation moves the expected result beyond the bound, or flips an index or a byte, on the inputs the GPU tests
     use -- so no GPU run is needed to see the GPU test fail."""
import numpy as np
import pytest
import torch

import scoring_fp64 as S
import vq_fp64 as R
from glare_amd import harness
from oracle import c_ref
from oracle import torch_ref as O


# ---- 1. VQ --------------------------------------------------------------------------------------------------------------------------------
def test_launch_shapes_and_counts():
    assert [R.slots_for(n) for n in (1, 128, 129, 32767, 32768)] == [64] * 5
    assert [R.slots_for(n) for n in (32769, 65535, 65536)] == [128] * 3
    assert [R.slots_for(n) for n in (65537, 65537 + 511, 130200)] == [256] * 3
    assert {R.parts_for(n) for n in R.SMALL_N} == {16}
    assert [R.parts_for(n) for n in R.LARGE_N] == [16, 16, 8, 8, 8, 4, 4, 4]
    assert (65537 + 510) % (256 * R.TPT) == 511 and (65537 + 511) % (256 * R.TPT) == 0 and 129 % (64 * R.TPT) == 1          # one token short, full, one over
    # fewer codes than ranges leave ranges empty; a chunk of one code belongs to the last range alone
    assert sum(hi > lo for lo, hi in R.ranges(7, 16)) == 7 and sum(hi > lo for lo, hi in R.ranges(3, 16)) == 3
    for parts in (16, 8, 4):
        assert [hi > lo for lo, hi in R.ranges(1, parts)] == [False] * (parts - 1) + [True]
        assert R.range_of(8192, 8193, parts) == (1, parts - 1) and R.range_of(16384, 16385, parts) == (2, parts - 1)
        for nc in (8192, 1000, 7, 3, 1):          # the ranges tile the chunk
            rs = R.ranges(nc, parts)
            assert rs[0][0] == 0 and rs[-1][1] == nc and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))


@pytest.mark.parametrize("k", (8192, 1000, 7))
def test_fp64_argmin_against_the_oracles_own_distances(k):
    z, cb = R.random(400, k)
    idx, zq, d = c_ref.vq_nearest(z, cb, return_d=True)
    ratio, best = R.excess(z, cb, idx)
    assert np.array_equal(best.numpy(), idx) and float(ratio.max()) == 0.0          # no near ties among random tokens
    d64 = ((z[:, None, :].astype(np.float64) - cb[None].astype(np.float64)) ** 2).sum(2)
    zz, ee = (z.astype(np.float64) ** 2).sum(1), (cb.astype(np.float64) ** 2).sum(1)
    assert bool((np.abs(d - d64) <= R.C_ROUND * R.U * (zz[:, None] + ee[None, :])).all())          # the count holds for EVERY code, not only the near ones
    assert np.array_equal(R.search_f32(z, cb), idx)
    assert np.array_equal(R.distances_f32(z, cb).astype(np.float32), d)          # the spelled roundings are the oracle's bits


@pytest.mark.parametrize("k", (8192, 1000, 8193))
def test_midpoint_family_decides_by_roundings(k):
    for name in ("midpoint0.7", "midpoint30", "midpoint_shifted"):
        z, cb = R.family(name, 3000, k)
        idx, _ = c_ref.vq_nearest(z, cb)
        ratio, best = R.excess(z, cb, idx)
        differ = float((torch.from_numpy(idx) != best).double().mean())
        assert differ >= 0.25, (name, k, differ)
        assert 0.0 < float(ratio.max()) < 1.0, (name, k, float(ratio.max()))
    z, cb = R.family("midpoint_shifted", 100, k)
    assert float((z.astype(np.float64) ** 2).sum(1).min()) > 1000.0          # zz + ee is far larger than a distance to a neighbour


@pytest.mark.parametrize("k", R.SMALL_K)
def test_oracle_stays_inside_the_counted_bound_on_every_family(k):
    for name in R.FAMILIES:
        z, cb = R.family(name, 129, k)
        idx, zq = c_ref.vq_nearest(z, cb)
        ratio, _ = R.excess(z, cb, idx)
        assert float(ratio.max()) < 1.0, (name, k, float(ratio.max()))
        if k <= 8193:
            assert np.array_equal(R.search_f32(z, cb), idx), (name, k)
        if name != "special":          # its plants sit at positions that follow from the listed counts: test_special_family
            head, cbh = R.family(name, 40, k)
            assert np.array_equal(S.bits32(head), S.bits32(z[:40])) and np.array_equal(S.bits32(cbh), S.bits32(cb)), name


@pytest.mark.parametrize("k", R.SMALL_K)
def test_duplicate_pairs_fall_in_different_ranges(k):
    pairs = R.duplicate_pairs(k)
    assert (len(pairs) > 0) == (k > 1)
    z, cb, lower = R.duplicate(129, k)
    for lo, hi in pairs:
        assert lo < hi and np.array_equal(S.bits32(cb[lo]), S.bits32(cb[hi]))
        for parts in (16, 8, 4):
            assert R.range_of(lo, k, parts) != R.range_of(hi, k, parts), (k, lo, hi, parts)
    if k == 16385:
        assert any(R.range_of(lo, k, 4)[0] != R.range_of(hi, k, 4)[0] for lo, hi in pairs)          # different resident chunks
        assert (k - 1) in [hi for _, hi in pairs]                                                    # ... the third chunk's only code too
        assert sum(hi == lo + 8192 for lo, hi in pairs) >= 40
    if k > 1:
        idx, _ = c_ref.vq_nearest(z, cb)
        assert np.array_equal(idx, lower) and len(set(lower.tolist())) == len(pairs)
        assert np.array_equal(S.bits32(z), S.bits32(cb[lower]))          # the tokens equal those rows


def test_special_family():
    z, cb = R.special(129, 1000)
    assert np.isnan(z[0]).all() and np.isnan(z[64]).all() and np.isposinf(z[128, 2]) and np.isneginf(z[43, 0])
    assert np.isnan(cb[500]).all() and np.isnan(cb[999, 1]) and np.isfinite(cb[:500]).all()
    idx, zq = c_ref.vq_nearest(z, cb)
    assert idx[0] == 0 and idx[64] == 0
    assert np.isfinite(cb[idx[np.isfinite(z).all(1)]]).all()
    assert np.array_equal(R.search_f32(z, cb), idx)
    plants = R.special_plants(max(R.LARGE_N))          # the GPU test cuts the family at the largest count to every listed one
    assert plants[0] == "nan" and all(m - 1 in plants and m // 2 in plants and m // 3 in plants for m in R.SMALL_N + R.LARGE_N if m > 3)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_vq_mutations_flip_an_index(mutation):
    """on the inputs of the GPU test: the duplicate family sees the merge, the midpoint family the roundings, any family a dropped range"""
    flipped = {}
    for name in ("random", "midpoint0.7", "duplicate"):
        for launch_n in (129, 32769, 65537):          # 16, 8 and 4 parts
            z, cb = R.family(name, 600, 1000)
            flipped[name, launch_n] = int((R.search_f32(z, cb, launch_n, mutation) != R.search_f32(z, cb, launch_n)).sum())
    if mutation == "last_range_skipped":
        assert all(v > 0 for (name, _), v in flipped.items() if name != "duplicate"), flipped          # (the lower copy of a pair is never in the last range)
    elif mutation == "merge_keeps_higher_index":
        assert all(flipped["duplicate", n] == 600 for n in (129, 32769, 65537)), flipped
        assert all(flipped["random", n] == 0 for n in (129, 32769, 65537))          # only a tie shows it: random inputs have none
    else:
        assert all(flipped["midpoint0.7", n] > 0 for n in (129, 32769, 65537)), flipped
        assert all(flipped["random", n] == 0 for n in (129, 32769, 65537))          # ... and only a near tie shows an fma


# ---- 2. pre / post-processing ---------------------------------------------------------------------------------------------------------------
def test_pre_table_and_index_maps(golden):
    g = golden("harness")
    table = S.pre_table64()
    img = g["img"][None]
    H, W = img.shape[1:3]
    ys, xs = S.pad_indices(H, 0, S.PAD, "reflect"), S.pad_indices(W, S.PAD, 0, "reflect")
    want = S.pre_expected(table, img, ys, xs)
    assert np.abs(want - g["pre"]).max() <= 3e-7 + 3e-7 * np.abs(want).max()
    assert np.abs(want - harness.preprocess(g["img"]).numpy()).max() <= 3e-7 + 3e-7 * np.abs(want).max()
    # fold() is np.pad's map, at every geometry the GPU test runs
    for B, H, W in S.PAIRED_SHAPES:
        assert np.array_equal(S.fold(np.arange(H + S.PAD), H, "reflect"), S.pad_indices(H, 0, S.PAD, "reflect"))
        assert np.array_equal(S.fold(np.arange(W + S.PAD) - S.PAD, W, "reflect"), S.pad_indices(W, S.PAD, 0, "reflect"))
    for H, W, (t, b, l, r) in S.PAD_CASES:
        for mode in ("reflect", "symmetric"):
            assert np.array_equal(S.fold(np.arange(H + t + b) - t, H, mode), S.pad_indices(H, t, b, mode))
            assert np.array_equal(S.fold(np.arange(W + l + r) - l, W, mode), S.pad_indices(W, l, r, mode))
    assert any(max(t, b) > 2 * H for H, W, (t, b, l, r) in S.PAD_CASES) and any(max(l, r) > 2 * W for H, W, (t, b, l, r) in S.PAD_CASES)
    # sensitivity: the period-2n fold differs wherever the pad is folded at all
    for B, H, W in S.PAIRED_SHAPES:
        assert not np.array_equal(S.fold(np.arange(H + S.PAD), H, "reflect", "fold_period_2n"), S.pad_indices(H, 0, S.PAD, "reflect"))
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, size=(1, 7, 33, 3)).astype(np.uint8)
    ys = S.fold(np.arange(7 + S.PAD), 7, "reflect", "fold_period_2n")
    xs = S.pad_indices(33, S.PAD, 0, "reflect")
    t32 = table.astype(np.float32)
    good = S.pre_expected(t32, img, S.pad_indices(7, 0, S.PAD, "reflect"), xs)
    assert not np.array_equal(S.bits32(S.pre_expected(t32, img, ys, xs)), S.bits32(good))


@pytest.mark.parametrize("shape", ((3, 20, 36), (2, 127, 129)))
def test_post_restatement_against_the_host_harness(shape, golden):
    B, h, w = shape
    out, gt = S.post_inputs(B, h, w, seed=w)
    ref = S.post_fp64(out, gt, h, w)
    for b in range(B):
        want = harness.postprocess(torch.from_numpy(out[b:b + 1, :, :, :S.PAD + w]), h, gt[b])          # the host form, fp32 numpy
        assert want.shape == (h, w, 3)
        assert np.abs(ref["restored"][b] - want).max() < 2e-6
        assert abs(ref["psnr"][b] - harness.psnr(gt[b] / 255.0, want)) < 1e-4
        assert abs(ref["psnr"][b] - harness.psnr(gt[b] / 255.0, ref["restored"][b])) < 1e-9
    assert bool((ref["bound"] > 0).all()) and float(ref["bound"].max()) < 1e-4 and float(ref["psnr_bound"].max()) < 1e-4
    assert ref["nonfinite"].tolist() == [0] * B
    g = golden("harness")
    assert abs(harness.psnr(g["a"], g["b"]) - float(g["psnr"])) < 1e-9
    d = g["a"] - g["b"]
    assert abs(10 * np.log10(1.0 / (d * d).mean()) - float(g["psnr"])) < 1e-9          # the form post_fp64 spells


def test_post_specials_and_mutations():
    B, h, w = S.POST_SHAPES[0]
    out, gt = S.post_inputs(B, h, w, seed=1)
    clean = S.post_fp64(out, gt, h, w)
    inside = {0: ("nan", "+inf"), 63: ("nan", "-inf"), 64: ("nan", "+inf", "-inf")}
    ref = S.post_fp64(S.plant_specials(out, h, w, inside, (1, 30, 62)), gt, h, w)
    assert ref["nonfinite"].tolist() == [2] + [0] * 62 + [2, 3]
    for b in range(B):
        if b in inside:
            assert np.isnan(ref["restored"][b]).all() and np.isnan(ref["psnr"][b])
        else:
            assert np.array_equal(ref["restored"][b], clean["restored"][b]) and ref["psnr"][b] == clean["psnr"][b]
    mut = S.post_fp64(out, gt, h, w, mutation="gray_weights_bgr")
    assert float((np.abs(mut["restored"] - clean["restored"]) / clean["bound"]).max()) > 1000.0
    assert float((np.abs(mut["psnr"] - clean["psnr"]) / clean["psnr_bound"]).max()) > 1000.0
    # the adjust protocol's gain: raw means, RGB-ordered weights
    Bs, Hp, Wp, window = S.SECOND_TRIP
    x, gt_full = S.output_and_gt(Bs, Hp, Wp, special=False)
    x = (x + 0.6).numpy()
    gts = gt_full[:, :window[2], :window[3]].numpy()
    want = S.adjust_gain_fp64(x, gts, window).astype(np.float64)
    for m in S.MUTATIONS["gain"]:
        assert bool((np.abs(S.adjust_gain_fp64(x, gts, window, m) / want - 1) > 1e-5).all()), m          # ten times the test's 1e-6 (uniform ground truth: the channel means are close)


# ---- 3. rounding to uint8 -------------------------------------------------------------------------------------------------------------------
def test_ubyte_ties_exist_and_tell_the_rounding_modes_apart():
    ties = S.half_products()
    even, odd = [k for k in ties if k % 2 == 0], [k for k in ties if k % 2 == 1]
    assert len(even) >= 10 and len(odd) >= 10, (len(even), len(odd))
    for k, x in ties.items():
        assert np.float32(np.float64(x) * 255.0) == np.float32(k + 0.5)
        assert S.to_ubyte_expected(np.float32([x]))[0] == (k if k % 2 == 0 else k + 1)          # ties to even
    pool = S.ubyte_pool()
    assert pool.size < max(S.UBYTE_N) and np.isnan(pool).any() and (pool < 0).any() and (pool > 1).any() and np.signbit(pool[pool == 0]).any()
    for n in S.UBYTE_N:
        x = S.ubyte_inputs(n)
        want = S.to_ubyte_expected(x)
        assert x.shape == (n,) and want.min() >= 0 and want.max() <= 255 and bool((want == np.floor(want)).all())
        # skimage's img_as_ubyte on the clipped image: the independent spelling
        c = np.clip(np.where(np.isnan(x), np.float32(0), x), np.float32(0), np.float32(1))
        assert np.array_equal(want, np.rint(c * np.float32(255)).astype(np.float64))
    x = S.ubyte_inputs(255)          # the smallest run that holds the ties
    for m in S.MUTATIONS["rounding"]:
        assert (S.to_ubyte_expected(x, m) != S.to_ubyte_expected(x)).sum() >= 10, m
    assert S.to_ubyte_expected(np.float32([np.nan, -0.0, -1.0, 2.0, np.inf, -np.inf])).tolist() == [0, 0, 0, 255, 255, 0]


# ---- 4. SSIM ----------------------------------------------------------------------------------------------------------------------------------
def test_ssim_restatement_against_the_oracle(golden):
    g = golden("ssim_metric")
    tgt, res = g["target"], g["restored"]
    val, _ = S.ssim_metric_fp64(res[None], tgt[None])
    assert abs(float(val[0]) - O.ssim_utils2(tgt, res)) < 2e-6          # the window reaches the kernel as floats: U per tap
    assert abs(float(val[0]) - float(g["ssim"])) < 5e-6
    for shape in S.SSIM_SHAPES:
        for family in S.SSIM_FAMILIES:
            res32, gt = S.ssim_inputs(shape, family, sum(shape))
            x255 = S.to_ubyte_expected(res32)
            val, _ = S.ssim_metric_fp64(x255, gt)
            for b in range(shape[0]):
                assert abs(float(val[b]) - O.ssim_utils2(gt[b], x255[b].astype(np.uint8))) < 2e-6, (shape, family)
            if family == "identical":
                assert np.array_equal(x255, gt.astype(np.float64)) and float((val - 1).abs().max()) < 1e-12
            if family == "dark":
                assert gt.max() <= 8
            if family == "bright_flat":
                assert gt.min() >= 248 and gt.max() <= 252
    assert abs(sum(S.metric_window()) - 1) < 1e-6 and S.METRIC_C1 == np.float32(6.5025) and S.METRIC_C2 == np.float32(58.5225)


# ---- 5. the word-owning sums ----------------------------------------------------------------------------------------------------------------
def test_word_sums_and_their_mutations():
    for special in (True, False):
        x, gt = S.tiny_outputs(special)
        B, Hp, Wp, window = S.TINY_IMAGES
        flags = S.window_nonfinite(x.numpy(), window)
        assert flags.shape == (65, 27) and np.array_equal(S.word_sums(flags), flags.sum(1))
        u8, sse = harness.score_u8(x.numpy(), gt.numpy(), None, window)
        d = (u8.astype(np.int64) - gt.numpy().astype(np.int64)).reshape(B, -1)
        assert np.array_equal(S.word_sums(d * d), sse)
    x, gt = S.tiny_outputs(True)
    flags = S.window_nonfinite(x.numpy(), window)
    cnt = flags.sum(1)
    assert cnt[0] > 0 and cnt[63] > 0 and cnt[64] > 0 and cnt[64] != cnt[0] and cnt[1] > 0 and cnt[4] == 0
    starts = [(27 * b) % 4 for b in range(B)]
    assert sum(s != 0 for s in starts) >= 48          # most images start mid-word
    assert all(flags[b, :(4 - (27 * b) % 4) % 4].any() for b in (1, 2, 3, 62))          # specials in the bytes the previous image's word carries
    assert (4 - (27 * 64) % 4) % 4 == 0                                                 # image 64 starts a word: nothing spills across the 64-image boundary ...
    assert (4 - (27 * 63) % 4) % 4 == 3 and flags[63].any()                             # ... but image 63's own first bytes are carried by image 62's word
    u8, sse = harness.score_u8(x.numpy(), gt.numpy(), None, window)
    d = (u8.astype(np.int64) - gt.numpy().astype(np.int64)).reshape(B, -1)
    for m in S.MUTATIONS["finish"]:
        assert not np.array_equal(S.word_sums(flags, m), cnt), m
        assert not np.array_equal(S.word_sums(d * d, m), sse), m
    assert S.word_sums(flags, "second_block_dropped")[64] == cnt[0]
    # the second-trip case is what it says
    B2, Hp2, Wp2, (top, left, h, w) = S.SECOND_TRIP
    assert 3 * h * w == 131949 > 128 * 256 * 4 and h * w == 43983 > 32768 and top + h < Hp2 and left + w < Wp2


# ---- 6. LPIPS ---------------------------------------------------------------------------------------------------------------------------------
def _seeded_lpips():
    from glare_amd.synthetic import seeded_init_

    net = seeded_init_(O.LPIPSAlex(), 7).double().eval()
    with torch.no_grad():
        for lin in net.lins:
            lin.model[-1].weight.abs_()
    return net


def test_conv_and_tap_restatements_against_lpips_alex():
    net = _seeded_lpips()
    g = torch.Generator().manual_seed(3)
    in0 = torch.rand(2, 3, 67, 51, generator=g, dtype=torch.float64) * 2 - 1
    in1 = (in0 + torch.randn(2, 3, 67, 51, generator=g, dtype=torch.float64) * 0.2).clamp(-1, 1)
    with torch.no_grad():
        want = net(in0, in1).view(-1)
        sh, sc = net.scaling_layer.shift.view(-1), net.scaling_layer.scale.view(-1)
        total = torch.zeros(2, dtype=torch.float64)
        h = [in0, in1]
        for s, (idx, cin, cout, k, st, pd) in enumerate(O.LPIPSAlex.CONVS):
            conv = getattr(getattr(net.net, "slice%d" % (s + 1)), str(idx))
            if s in (1, 2):
                h = [torch.nn.functional.max_pool2d(a, 3, 2) for a in h]
            aff = dict(shift=sh, scale=sc) if s == 0 else {}
            outs = [S.conv_fp64(a, conv.weight, conv.bias, st, pd, relu=True, **aff) for a in h]
            assert all(bool((b > 0).all()) and bool(torch.isfinite(b).all()) for _, b in outs)
            h = [e for e, _ in outs]
            B, C = h[0].shape[:2]
            total += S.lpips_tap_fp64(h[0].reshape(B, C, -1), h[1].reshape(B, C, -1), net.lins[s].model[-1].weight.view(-1), eps=1e-10)
    assert float((total - want).abs().max()) < 1e-12 * float(want.abs().max()) + 1e-15
    assert float(want.min()) > 0


def test_lpips_mutations():
    # eps inside the square root is seen on SMALL feature vectors (|f| ~ 1e-4: sqrt(|f|^2 + 1e-10) against |f| + 1e-10); the GPU test scales
    # its second image down by the same factor
    f0, f1, lin = S.tap_inputs(2, 64, 257, seed=5)
    f0[1] *= S.TAP_SMALL
    f1[1] *= S.TAP_SMALL
    a, b = S.lpips_tap_fp64(f0, f1, lin), S.lpips_tap_fp64(f0, f1, lin, mutation="eps_inside_sqrt")
    assert abs(float(b[1] / a[1]) - 1) > 1e-3 and abs(float(b[0] / a[0]) - 1) < 1e-6
    # zero feature vectors: no NaN, the exact contribution
    f0, f1, lin = S.tap_inputs(1, 7, 5, seed=1)
    f0[:, :, 2:] = f1[:, :, 2:]          # only pixels 0 and 1 are left to contribute
    want = float(((f1[0, :, 0].double() / (f1[0, :, 0].double().norm() + S.LPIPS_EPS)) ** 2 * lin.double()).sum() / 5)
    got = float(S.lpips_tap_fp64(f0, f1, lin)[0])
    assert np.isfinite(got) and abs(got - want) <= 1e-15
    assert float(S.lpips_tap_fp64(f1, f1, lin)[0]) == 0.0
    # padding before the affine: the all-`shift` image no longer gives the bias
    sh, sc = torch.tensor([-.030, -.088, -.188]), torch.tensor([.458, .448, .450])
    x = sh.view(1, 3, 1, 1).expand(1, 3, 7, 7).contiguous()
    w = torch.randn(7, 3, 11, 11, generator=torch.Generator().manual_seed(0)) * 0.05
    bias = torch.randn(7, generator=torch.Generator().manual_seed(1))
    exact, bound = S.conv_fp64(x, w, bias, 4, 2, False, sh, sc)
    assert torch.equal(exact, bias.double().view(1, 7, 1, 1).expand_as(exact))
    mut, _ = S.conv_fp64(x, w, bias, 4, 2, False, sh, sc, mutation="pad_before_affine")
    assert float(((mut - exact).abs() / bound).max()) > 1000.0


def test_conv_cases_are_what_they_claim():
    chunk = lambda k: 8192 // (32 * k * k)
    assert [chunk(k) for k in (3, 5, 11, 16)] == [28, 10, 2, 1] and 32 * 17 * 17 > 8192
    for k, st, pd, cin in S.CONV_CIN:
        assert cin % chunk(k) != 0 or chunk(k) == 1          # a ragged last chunk (k = 16: one channel per chunk, three trips)
        assert cin > chunk(k)
    for k, st, pd in S.ALEX:
        for oh, ow in S.CONV_OHW:
            H, W = S.conv_input_size(oh, k, st, pd), S.conv_input_size(ow, k, st, pd)
            assert H >= 1 and W >= 1 and (H + 2 * pd - k) // st + 1 == oh and (W + 2 * pd - k) // st + 1 == ow
            assert H - 1 < 1 or (H - 1 + 2 * pd - k) // st + 1 < oh          # the smallest such side
    assert S.conv_input_size(1, 11, 4, 2) < 11          # H < k: reachable only through the padding
    assert sorted(oh * ow for oh, ow in S.CONV_OHW) == [1, 63, 65]
    # the bound is a bound: an fp32 evaluation in torch stays inside it
    g = torch.Generator().manual_seed(2)
    x, w, b = torch.randn(2, 29, 7, 9, generator=g), torch.randn(33, 29, 3, 3, generator=g) * 0.1, torch.randn(33, generator=g)
    exact, bound = S.conv_fp64(x, w, b, 1, 1, True)
    got = torch.relu(torch.nn.functional.conv2d(x, w, b, 1, 1)).double()
    assert float(((got - exact).abs() / bound).max()) < 1.0
