"""GPU: the two kernels of tiled enhancement (glare_harness_tile_gather_u8, glare_harness_tile_blend_f32) at small shapes -- the
gather bit for bit against the unpaired harness' pad-and-encode kernel wherever the two describe the same pixels, the blend byte for
byte against its crop-and-quantise kernel for a single window, and per element against the fp64 restatement (tile_fp64.py) on grids
with two and three windows over a coordinate."""
import numpy as np
import pytest
import torch

from glare_amd import enhance, harness

import tile_fp64 as T64

pytestmark = pytest.mark.gpu

MODES = [harness.PAD_SYMMETRIC, harness.PAD_REFLECT101]


def _gather(img, origins, th, tw, mode):
    o = torch.tensor(origins, dtype=torch.int32).cuda()
    return harness.tile_gather_device(torch.from_numpy(np.ascontiguousarray(img)).cuda(), o, th, tw, mode).cpu()


def _encode(img, pads, mode):
    return harness.preprocess_unpaired_device(torch.from_numpy(np.ascontiguousarray(img))[None].cuda(), pads, mode).cpu()


@pytest.mark.parametrize("mode", MODES)
def test_gather_whole_image_window_is_the_pad_kernel_bit_for_bit(mode):
    img = np.random.default_rng(1).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    p = harness.auto_padding(37, 53)
    got = _gather(img, [(-p[0], -p[2])], 37 + p[0] + p[1], 53 + p[2] + p[3], mode)
    want = _encode(img, p, mode)
    assert got.shape == want.shape == (1, 3, 48, 64)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_gather_interior_and_border_windows_are_crops():
    img = np.random.default_rng(2).integers(0, 256, (50, 70, 3), dtype=np.uint8)
    origins = [(0, 0), (0, 22), (18, 0), (18, 22), (9, 11)]                   # the four corners and the middle, 32 x 48
    got = _gather(img, origins, 32, 48, harness.PAD_SYMMETRIC)
    assert got.shape == (5, 3, 32, 48)
    for t, (y, x) in enumerate(origins):
        want = _encode(img[y:y + 32, x:x + 48], (0, 0, 0, 0), harness.PAD_SYMMETRIC)
        assert torch.equal(got[t:t + 1].view(torch.int32), want.view(torch.int32)), (y, x)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h,w,pads", [(1, 1, (4, 5, 6, 7)), (3, 5, (9, 13, 11, 6)), (1, 4, (3, 2, 9, 9))])
def test_gather_folds_past_the_image_as_the_pad_kernel(h, w, pads, mode):
    img = np.random.default_rng(h * 10 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = _gather(img, [(-pads[0], -pads[2])], h + pads[0] + pads[1], w + pads[2] + pads[3], mode)
    assert torch.equal(got.view(torch.int32), _encode(img, pads, mode).view(torch.int32))


def _plan(H, W, T, O):
    """A plan dict as harness.tile_blend_device takes it, from the fp64 module's starts (ramps narrower than 16 allowed)."""
    (ys, th), (xs, tw) = T64.axis_plan(H, T, O), T64.axis_plan(W, T, O)
    return {"h": H, "w": W, "tile": T, "overlap": O, "ys": ys, "xs": xs, "th": th, "tw": tw,
            "row_table": enhance.axis_weights(H, ys, th, O), "col_table": enhance.axis_weights(W, xs, tw, O)}


def _blend(tiles, plan):
    u8, f32, bad = harness.tile_blend_device(tiles.cuda(), plan, want_f32=True)
    return u8.cpu().numpy(), f32.cpu().numpy(), int(bad.cpu())


def _oracle(tiles, plan):
    return T64.blend64(tiles.numpy(), plan["ys"], plan["xs"], plan["h"], plan["w"], plan["th"], plan["tw"], plan["overlap"])


@pytest.mark.parametrize("Hp,Wp,pads,h,w", [(16, 16, (3, 4, 5, 2), 9, 9), (32, 48, (8, 8, 8, 8), 16, 32), (13, 11, (0, 0, 0, 0), 13, 11),
                                            (16, 16, (7, 8, 7, 8), 1, 1)])
def test_blend_of_a_single_window_is_postprocess_u8_byte_for_byte(Hp, Wp, pads, h, w):
    g = torch.Generator().manual_seed(Hp * Wp + 1)            # the inputs of test_postprocess_u8_is_rgb_of_the_crop_bit_for_bit
    x = torch.rand(1, 3, Hp, Wp, generator=g, dtype=torch.float64).mul(1.4).sub(0.2).float()
    k = torch.randint(0, 256, x.shape, generator=g).float() / 255          # on k/255 and one ulp either side
    sel = torch.rand(x.shape, generator=g)
    x = torch.where(sel < 0.3, k, x)
    x = torch.where((sel >= 0.3) & (sel < 0.4), torch.nextafter(k, torch.tensor(2.0)), x)
    x = torch.where((sel >= 0.4) & (sel < 0.5), torch.nextafter(k, torch.tensor(-1.0)), x)
    flat = x.view(-1)
    spec = torch.randint(0, flat.numel(), (max(3, flat.numel() // 50),), generator=g)
    for j, i in enumerate(spec.tolist()):
        flat[i] = (float("nan"), float("inf"), float("-inf"))[j % 3]
    plan = {"h": h, "w": w, "ys": [-pads[0]], "xs": [-pads[2]], "th": Hp, "tw": Wp,
            "row_table": enhance.axis_weights(h, [-pads[0]], Hp, 16), "col_table": enhance.axis_weights(w, [-pads[2]], Wp, 16)}
    assert (plan["row_table"][2][:, 0] == 1).all() and (plan["col_table"][2][:, 0] == 1).all()
    u8, f32, bad = _blend(x, plan)
    want, want_bad = harness.postprocess_unpaired_device(x.cuda(), pads, h, w, want_nonfinite=True)
    assert np.array_equal(u8, want.cpu().numpy()[0])
    assert bad == int(want_bad.cpu()[0])
    crop = x[0, :, pads[0]:pads[0] + h, pads[2]:pads[2] + w].permute(1, 2, 0).numpy()
    assert np.array_equal(u8, harness.rgb_u8(crop)) and bad == int((~np.isfinite(crop)).sum())
    assert np.array_equal(f32, np.clip(np.where(np.isnan(crop), np.float32(0), crop), np.float32(0), np.float32(1)))


GRIDS = [(61, 90, 32, 8), (33, 33, 32, 16), (96, 112, 64, 16)]


def _random_tiles(plan, seed):
    g = torch.Generator().manual_seed(seed)
    n = len(plan["ys"]) * len(plan["xs"])
    return torch.rand(n, 3, plan["th"], plan["tw"], generator=g, dtype=torch.float64).mul(1.4).sub(0.2).float()


@pytest.mark.parametrize("H,W,T,O", GRIDS)
def test_blend_of_a_grid_against_fp64(H, W, T, O, capsys):
    plan = _plan(H, W, T, O)
    if (H, W) == (61, 90):
        assert plan["ys"] == [0, 24, 29] and len(plan["xs"]) == 4 and int(plan["row_table"][1][29:32].min()) == 3
    tiles = _random_tiles(plan, H * W)
    u8, f32, bad = _blend(tiles, plan)
    acc, want_bad = _oracle(tiles, plan)
    err = float(np.abs(f32.astype(np.float64) - acc).max())
    wrong, share = T64.u8_mismatch(u8, acc)
    with capsys.disabled():
        print("\n[tile blend %dx%d T=%d O=%d] max |fp32 - fp64| = %.2f * 2^-24 (bound 16), uint8 off-by-one at a step: %.4f %% (cap 0.5)"
              % (H, W, T, O, err * 2.0 ** 24, 100 * share))
    assert bad == want_bad == 0
    assert err <= T64.BOUND
    assert wrong == 0
    assert share <= T64.U8_CAP


@pytest.mark.parametrize("c", [0.0, 0.3, 1.0])
def test_blend_of_constant_windows_is_the_constant(c):
    for H, W, T, O in GRIDS:
        plan = _plan(H, W, T, O)
        n = len(plan["ys"]) * len(plan["xs"])
        u8, f32, bad = _blend(torch.full((n, 3, plan["th"], plan["tw"]), c, dtype=torch.float32), plan)
        assert bad == 0
        assert float(np.abs(f32.astype(np.float64) - float(np.float32(c))).max()) <= T64.BOUND
        if c in (0.0, 1.0):
            assert (u8 == int(c) * 255).all() or (c == 1.0 and u8.min() >= 254)      # 1 - a few ulp truncates to 254


def test_blend_counts_nonfinite_values_inside_the_image_once_per_window():
    plan = _plan(20, 90, 32, 16)          # rows: one padded window [-6, 26); columns: windows 0, 16, 32, 48, 58 -- three cover 58..63
    assert plan["ys"] == [-6] and plan["th"] == 32 and plan["xs"] == [0, 16, 32, 48, 58]
    tiles = _random_tiles(plan, 7)
    nan, inf = float("nan"), float("inf")
    tiles[0, 0, 2, 5] = nan               # a pad row (image row -4): not counted
    tiles[1, 1, 31, 3] = inf              # a pad row (image row 25)
    tiles[4, 2, 0, 31] = -inf             # a pad row
    tiles[0, 0, 6, 20] = nan              # image (0, 20): windows 0 and 1 cover it; planted in window 0 only -> 1
    tiles[1, 1, 10, 4] = inf              # image (4, 20), window 1 -> 1
    tiles[2, 2, 12, 30] = -inf            # image (6, 62): windows 2, 3 and 4 cover it
    tiles[3, 2, 12, 14] = inf             # ... the same value position in window 3 -> counted again
    tiles[4, 2, 12, 4] = nan              # ... and in window 4
    tiles[4, 0, 25, 31] = nan             # image (19, 89): the last pixel, one window
    u8, f32, bad = _blend(tiles, plan)
    acc, want_bad = _oracle(tiles, plan)
    assert want_bad == 6 and bad == want_bad
    assert np.isfinite(f32).all()
    assert float(np.abs(f32.astype(np.float64) - acc).max()) <= T64.BOUND
    assert T64.u8_mismatch(u8, acc)[0] == 0


def test_blend_is_repeatable():
    plan = _plan(61, 90, 32, 8)
    tiles = _random_tiles(plan, 11)
    tiles[3, 1, 4, 4] = float("inf")
    a, b = _blend(tiles, plan), _blend(tiles, plan)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] == 1


def test_bad_arguments_are_refused():
    from glare_amd import _lib

    img = torch.zeros(4, 4, 3, dtype=torch.uint8).cuda()
    with pytest.raises(_lib.GlareError) as ei:
        harness.tile_gather_device(img, torch.zeros(1, 2, dtype=torch.int32).cuda(), 8, 8, mode=7)
    assert ei.value.status == _lib.ERR_INVALID
