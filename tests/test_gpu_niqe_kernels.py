"""GPU: the four NIQE kernels (csrc/niqe.hip) per element against the fp64 restatement (tests/niqe_fp64.py).  Luma and the counts are
exact; every other bound is the fp32 (moments: fp64) evaluation error of the kernel's own expression, counted from its source in the
style of fp64_bounds.py (U = 2^-24 per fp32 rounding) and passed through tolerances.within as measured / bound < 1."""
import math

import numpy as np
import pytest
import torch

import niqe_fp64 as N
from fp64_bounds import U, assert_f32
from glare_amd import _lib, metrics
from tolerances import within

pytestmark = pytest.mark.gpu

WINDOW = N.synthetic_params()["gaussian_window"]
U64 = 2.0 ** -53


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


# ---- luma -------------------------------------------------------------------------------------------------------------------------
def test_luma_of_every_colour_is_the_exact_rule():
    """All 2^24 colours as a 4096 x 4096 image, set into a 4128 x 4128 one (43 whole blocks a side) so that the crop keeps them all."""
    g = np.arange(256, dtype=np.uint8)
    colours = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(4096, 4096, 3)
    img = np.pad(colours, ((0, 32), (0, 32), (0, 0)), mode="edge")
    got = metrics.niqe_luma(torch.from_numpy(img[None]).cuda())[0].cpu().numpy()
    assert got.shape == (4128, 4128) and got.dtype == np.float32
    assert np.array_equal(got.astype(np.int64), N.luma(img))


def test_luma_crops_to_whole_blocks():
    img = np.random.default_rng(1).integers(0, 256, (2, 100, 203, 3), dtype=np.uint8)
    got = metrics.niqe_luma(torch.from_numpy(img).cuda()).cpu().numpy()
    assert got.shape == (2, 96, 192)
    assert np.array_equal(got.astype(np.int64), N.luma(img)[:, :96, :192])


# ---- mscn -------------------------------------------------------------------------------------------------------------------------
def _patch_sums(y, window):
    """Per pixel, about its own value c: S1 = sum w d, A = sum w |d|, Q = sum w d^2 over the replicated 7 x 7 patch, d = y - c (fp64)."""
    H, W = y.shape
    p = np.pad(y, 3, mode="edge")
    S1, A, Q = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    for a in range(7):
        for b in range(7):
            d = p[6 - a:6 - a + H, 6 - b:6 - b + W] - y
            S1 += window[a, b] * d
            A += window[a, b] * np.abs(d)
            Q += window[a, b] * d * d
    return S1, A, Q


def _mscn_bound(y, window):
    """niqe_mscn_kernel, rounding by rounding.  d = fl(v - c): U |d|.  wd = fl(w32 d), w32 = fl(w): 3 U with d's.  S1: 49 terms added in
    sequence, 48 U sum |wd|: E1 = 52 U A (one U for the second order).  S2 = fma(wd, d, S2): 4 U per term and 49 U Q for the running
    sum of positive terms: E2 = 54 U Q.  num = fma(c, oms0, -S1): E1 + U |num| + U |c oms0|.  var = fl(fl(S2 - fl(S1^2)) + fl(oms0 (...))):
    E2 + 2 |S1| E1 + E1^2 + 3 U (Q + S1^2) + 6 U |oms0| (c^2 + 2 |c S1|).  sigma = fl(sqrt |var|): min(sqrt Ev, Ev / sigma) + U sigma.  den = fl(sigma + 1): + U den.
    n = fl(num / den): (E_num + |n| E_den) / max(1, den - E_den) + 2 U |n|."""
    s0, oms0 = metrics.niqe_window_sums(window)
    S1, A, Q = _patch_sums(y, window)
    E1, E2 = 52 * U * A, 54 * U * Q
    num = y * oms0 - S1
    var = Q - S1 * S1 + oms0 * (y * y * s0 + 2 * y * S1)
    sigma = np.sqrt(np.abs(var))
    n = num / (sigma + 1)
    e_num = E1 + U * np.abs(num) + U * np.abs(y * oms0)
    e_var = E2 + 2 * np.abs(S1) * E1 + E1 * E1 + 3 * U * (Q + S1 * S1) + 6 * U * abs(oms0) * (y * y + 2 * np.abs(y * S1))
    with np.errstate(divide="ignore", invalid="ignore"):
        e_sig = np.minimum(np.sqrt(e_var), np.where(sigma > 0, e_var / sigma, np.inf)) + U * sigma
    e_den = e_sig + U * (sigma + 1)
    return (e_num + np.abs(n) * e_den) / np.maximum(1.0, sigma + 1 - e_den) + 2 * U * np.abs(n) + 1e-30


def _smooth(rng, B, H, W):
    """Integer luma like a photograph's: a smooth field plus texture, 16..235."""
    coarse = rng.uniform(30, 220, (B, H // 8 + 2, W // 8 + 2))
    yy, xx = np.arange(H) / 8.0, np.arange(W) / 8.0
    y0, x0 = yy.astype(int), xx.astype(int)
    fy, fx = (yy - y0)[None, :, None], (xx - x0)[None, None, :]
    c = lambda dy, dx: coarse[:, y0 + dy][:, :, x0 + dx]
    field = (1 - fy) * ((1 - fx) * c(0, 0) + fx * c(0, 1)) + fy * ((1 - fx) * c(1, 0) + fx * c(1, 1))
    return np.clip(np.round(field + rng.normal(0, 6, (B, H, W))), 16, 235)


@pytest.mark.parametrize("name,B,H,W", [("smaller than the halo", 1, 7, 9), ("one block", 1, 96, 96), ("odd, batch of 2", 2, 97, 131),
                                        ("flat plus one level of noise", 1, 48, 80), ("non-integer", 1, 33, 70)])
def test_mscn_against_fp64(name, B, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    if name.startswith("flat"):                   # the cancellation case: E[y^2] - mu^2 in fp32 would lose 0.004, the variance is <= 0.25
        y = 250.0 + rng.integers(0, 2, (B, H, W)).astype(np.float64)
    elif name == "non-integer":                   # the second scale's input is not integer-valued
        y = _smooth(rng, B, H, W) + rng.uniform(-0.5, 0.5, (B, H, W))
        y = y.astype(np.float32).astype(np.float64)
    else:
        y = _smooth(rng, B, H, W)
    got = metrics.niqe_mscn(_dev(y), WINDOW).cpu()
    for b in range(B):
        want = N.mscn(y[b], WINDOW)
        r = assert_f32(got[b], torch.from_numpy(want), torch.from_numpy(_mscn_bound(y[b], WINDOW)), "mscn %s" % name)
        print("mscn %s [%d]: worst measured / bound %.3f, max |n| %.3f" % (name, b, r, float(np.abs(want).max())))
    if name.startswith("flat"):                   # ... and the result is far from what the cancelling form gives
        naive = N.mscn(y[0], WINDOW, storage=np.float32)
        assert float(np.abs(naive - N.mscn(y[0], WINDOW)).max()) > 50 * float((got[0].double() - torch.from_numpy(N.mscn(y[0], WINDOW))).abs().max())


def test_mscn_of_a_constant_image_is_exactly_zero():
    y = torch.full((2, 40, 70), 201.0, device="cuda")
    got = metrics.niqe_mscn(y, WINDOW)
    assert int(torch.count_nonzero(got)) == 0 and not bool(torch.signbit(got).any())


def test_mscn_with_a_window_that_does_not_sum_to_one():
    """one_minus_s0 carries the rest of the variance: 0.75 of the window."""
    y = _smooth(np.random.default_rng(5), 1, 40, 72)[0]
    w = WINDOW * 0.75
    got = metrics.niqe_mscn(_dev(y[None]), w).cpu()[0]
    assert_f32(got, torch.from_numpy(N.mscn(y, w)), torch.from_numpy(_mscn_bound(y, w)), "mscn window sum 0.75")


# ---- block moments ----------------------------------------------------------------------------------------------------------------
def _check_moments(n32, bh, bw, tag):
    """Counts exact.  Sums: products of two fp32 values are exact in fp64, a square costs one rounding; a lane adds ceil(bh bw / 256)
    terms in sequence, the butterfly 6 more, the wave partials 3: (ceil(bh bw / 256) + 10) 2^-53 relative to a sum of positive terms."""
    got = metrics.niqe_block_moments(torch.from_numpy(n32).cuda(), bh, bw).cpu().numpy()
    B, H, W = n32.shape
    assert got.shape == (B, W // bw, H // bh, 5, 5)
    rel = (math.ceil(bh * bw / 256) + 10) * U64
    worst = 0.0
    for b in range(B):
        want = N.block_moments(n32[b].astype(np.float64), bh, bw)
        assert np.array_equal(got[b][..., :2], want[..., :2]), tag
        err = np.abs(got[b][..., 2:] - want[..., 2:]) / (rel * want[..., 2:] + 1e-300)
        worst = max(worst, float(err.max()))
    print("moments %s: worst measured / bound %.3f" % (tag, worst))
    return within(worst, 1.0, "moments " + tag)


def test_moments_small_blocks():
    n = np.random.default_rng(7).standard_normal((2, 24, 36)).astype(np.float32)
    _check_moments(n, 8, 12, "8x12 on 24x36")


def test_moments_full_blocks_and_an_empty_side():
    rng = np.random.default_rng(8)
    n = rng.standard_normal((1, 96, 192)).astype(np.float32)
    n[0, :, 96:] = np.abs(n[0, :, 96:]) + 0.01                     # the second block has no negative value, in any of the five maps
    _check_moments(n, 96, 96, "96x96 on 96x192")
    got = metrics.niqe_block_moments(torch.from_numpy(n).cuda()).cpu().numpy()[0]
    assert (got[1, 0, :, 0] == 0).all() and (got[1, 0, :, 1] == 9216).all() and (got[1, 0, :, 2] == 0).all()
    assert (got[0, 0, :, 0] > 0).all() and (got[0, 0, :, 0] + got[0, 0, :, 1] == 9216).all()


def test_moments_shifts_are_np_roll_inside_the_block():
    """Blocks whose products tell the four shifts apart, and a shift that left its block from one that wrapped inside it: every block of
    the 2 x 3 grid has its own scale.  (A shift and its opposite give the same products in another order, hence the same moments.)"""
    bh, bw = 6, 10
    i, j = np.meshgrid(np.arange(bh), np.arange(bw), indexing="ij")
    block = (1.0 + i + 100.0 * j) * np.where((i + j) % 3 == 0, -1.0, 1.0)
    n = (np.tile(block, (2, 3)) * np.kron(np.array([[1.0, 3.0, 5.0], [2.0, 6.0, 10.0]]), np.ones((bh, bw)))).astype(np.float32)[None]
    got = metrics.niqe_block_moments(torch.from_numpy(n).cuda(), bh, bw).cpu().numpy()[0]
    for bx in range(3):
        for by in range(2):
            blk = n[0, by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw].astype(np.float64)
            want = [N.map_moments(blk * np.roll(blk, s, axis=(0, 1))) for s in N.SHIFTS]
            for m, s in enumerate(N.SHIFTS):
                assert all(np.abs(want[o] - want[m]).max() >= 1 for o in range(4) if o != m)      # the moments tell the shifts apart
                assert np.array_equal(got[bx, by, m + 1, :2], want[m][:2])
                np.testing.assert_allclose(got[bx, by, m + 1, 2:], want[m][2:], rtol=16 * U64)


# ---- halve ------------------------------------------------------------------------------------------------------------------------
def _halve_abs(y):
    """The two passes with |tap| on |y|: an upper bound of sum |tap| |t| of the W pass and of the carried H-pass error."""
    saved = N.TAPS.copy()
    try:
        N.TAPS[:] = np.abs(saved)
        return N.halve(np.abs(y))
    finally:
        N.TAPS[:] = saved


@pytest.mark.parametrize("B,H,W", [(1, 4, 4), (2, 8, 10), (1, 96, 192), (1, 34, 130)])
def test_halve_against_fp64(B, H, W):
    """The taps are exact in fp32.  A pass is one rounded product and seven fmaf: 8 U sum |tap v|.  The W pass carries the H pass's error
    through |tap| and adds its own on the rounded intermediates: 16 U P, P = the two passes with |tap| on |y|; 17 for the second order."""
    y = np.random.default_rng(H * W).uniform(0, 255, (B, H, W)).astype(np.float32)
    got = metrics.niqe_halve(torch.from_numpy(y).cuda()).cpu()
    assert got.shape == (B, H // 2, W // 2)
    for b in range(B):
        y64 = y[b].astype(np.float64)
        r = assert_f32(got[b], torch.from_numpy(N.halve(y64)), torch.from_numpy(17 * U * _halve_abs(y64)), "halve %dx%d" % (H, W))
        print("halve %dx%d [%d]: worst measured / bound %.3f" % (H, W, b, r))


@pytest.mark.parametrize("H,W", [(5, 8), (8, 7), (2, 8), (8, 2), (3, 3)])
def test_halve_refuses_odd_and_small_sizes(H, W):
    with pytest.raises(_lib.GlareError) as ei:
        metrics.niqe_halve(torch.zeros(1, H, W, device="cuda"))
    assert ei.value.status == _lib.ERR_INVALID


def test_kernels_repeat_bit_for_bit():
    rng = np.random.default_rng(9)
    img = torch.from_numpy(rng.integers(0, 256, (2, 192, 200, 3), dtype=np.uint8)).cuda()
    runs = []
    for _ in range(2):
        y = metrics.niqe_luma(img)
        n = metrics.niqe_mscn(y, WINDOW)
        y2 = metrics.niqe_halve(y)
        runs.append([y, n, metrics.niqe_block_moments(n), y2, metrics.niqe_block_moments(metrics.niqe_mscn(y2, WINDOW), 48, 48)])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))
