"""CPU: the tile plan of glare_amd.enhance (plan_axis, axis_weights, plan_tiles) against its contract and the fp64 restatement in
tile_fp64.py, and the tiled driver with a stub network and the fp64 blend."""
import numpy as np
import pytest

from glare_amd import enhance, harness

import tile_fp64 as T64

_TO = [(32, 16), (64, 16), (512, 64)]


def _lengths(tile, overlap):
    return [1, 15, 16, 17, tile, tile + 1, 2 * tile - overlap, 2 * tile - overlap + 1, 1000]


@pytest.mark.parametrize("tile,overlap", _TO)
def test_plan_axis_covers_the_axis(tile, overlap):
    for L in _lengths(tile, overlap):
        starts, length, keep0 = enhance.plan_axis(L, tile, overlap)
        n = len(starts)
        assert (starts, length) == tuple(T64.axis_plan(L, tile, overlap)), L
        cover = np.zeros(L, dtype=int)
        for s in starts:
            cover[max(s, 0):min(s + length, L)] += 1
        assert cover.min() >= 1 and cover.max() <= 3, (L, starts)                     # every coordinate, by at most 3 windows
        if L <= tile:                                                                  # one window: the untiled path's padding
            p1, p2 = harness.auto_padding(L, 40)[:2]
            assert n == 1 and starts == [-p1] and length == L + p1 + p2 and keep0 == p1 and length % 16 == 0
            assert (p1, p2) == harness.auto_padding(40, L)[2:]
        else:
            assert n > 1 and length == tile and keep0 == 0
            assert starts[0] == 0 and starts[-1] + tile == L and all(0 <= s and s + tile <= L for s in starts)
            assert all(b > a for a, b in zip(starts, starts[1:]))
            assert all(a + tile - b >= overlap for a, b in zip(starts, starts[1:])), (L, starts)
            assert n == -(-(L - overlap) // (tile - overlap))


@pytest.mark.parametrize("L,tile,overlap", [(100, 24, 16), (100, 0, 16), (100, 32, 8), (100, 32, 15), (100, 32, 17), (100, 64, 33),
                                            (0, 32, 16), (100, -32, 16)])
def test_plan_axis_refuses_bad_arguments(L, tile, overlap):
    with pytest.raises(ValueError):
        enhance.plan_axis(L, tile, overlap)
    with pytest.raises(ValueError):
        enhance.plan_tiles(L, 50, tile, overlap)


@pytest.mark.parametrize("tile,overlap", _TO)
def test_axis_weights_follow_the_contract(tile, overlap):
    for L in _lengths(tile, overlap):
        starts, length, _ = enhance.plan_axis(L, tile, overlap)
        first, count, weight = enhance.axis_weights(L, starts, length, overlap)
        assert first.dtype == np.int32 and count.dtype == np.int32 and weight.dtype == np.float32 and weight.shape == (L, 3)
        want = T64.axis_weights64(L, starts, length, overlap)                # [n][L], 0 where a window does not cover x
        dense = np.zeros_like(want)
        for x in range(L):
            assert 1 <= count[x] <= 3 and 0 <= first[x] and first[x] + count[x] <= len(starts)
            for a in range(3):
                if a < count[x]:
                    dense[first[x] + a, x] = weight[x, a]
                else:
                    assert weight[x, a] == 0
        assert np.array_equal(dense > 0, want > 0), L                           # exactly the covering windows
        assert np.array_equal(dense, want.astype(np.float32).astype(np.float64)), L     # fp64, rounded once
        assert np.abs(weight.astype(np.float64).sum(axis=1) - 1).max() <= 2.0 ** -23
        if len(starts) == 1:
            assert (weight[:, 0] == np.float32(1)).all() and (count == 1).all()
        else:                                                                   # no seam: a window fades to 0.5 / O at its cut edges
            for i, s in enumerate(starts):
                if i > 0:
                    assert want[i, s] <= 0.5 / overlap + 1e-12
                if i < len(starts) - 1:
                    assert want[i, s + length - 1] <= 0.5 / overlap + 1e-12


def test_plan_tiles_keeps_every_window_inside_the_envelope():
    plan = enhance.plan_tiles(2160, 3840, 512, 64)
    assert (plan["th"], plan["tw"]) == (512, 512) and (len(plan["ys"]), len(plan["xs"])) == (5, 9)
    enhance.check_size(plan["th"], plan["tw"], 1)
    assert enhance.max_batch(plan["th"], plan["tw"]) >= 8
    with pytest.raises(ValueError):
        enhance.check_size(2176, 3856)                                          # the same image, untiled
    mixed = enhance.plan_tiles(300, 1000, 512, 64)                               # one padded window down, tiles across
    assert mixed["ys"] == [-2] and mixed["th"] == 304 and mixed["tw"] == 512 and mixed["keep"] == (2, 0)
    with pytest.raises(ValueError, match="huge.png"):                           # a tile shape outside the envelope: before any launch
        enhance.plan_tiles(3000, 3000, 2048, 64, name="huge.png")


def _stub_tile_fn(calls):
    """A stand-in network: undoes the log transform, so a window's 'output' is its input image / 255."""
    def fn(lr, precision):
        lr = np.asarray(lr, dtype=np.float64)
        calls.append((lr.shape, precision))
        return (np.exp(lr) - 1e-3).astype(np.float32)
    return fn


def _fp64_blend_fn(tiles, plan):
    acc, bad = T64.blend64(tiles, plan["ys"], plan["xs"], plan["h"], plan["w"], plan["th"], plan["tw"], plan["overlap"])
    return np.floor(np.minimum(acc, 1.0) * 255.0).astype(np.uint8), bad


@pytest.mark.parametrize("h,w,tile,overlap,grid", [(70, 100, 32, 16, (4, 6)), (20, 75, 32, 16, (1, 4)), (30, 30, 32, 16, (1, 1)),
                                                   (33, 33, 32, 16, (2, 2))])
def test_enhance_tiled_on_the_host_returns_the_input(h, w, tile, overlap, grid):
    rng = np.random.default_rng(h * 1000 + w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    calls, rep = [], {}
    out = enhance.enhance_tiled(img, tile=tile, overlap=overlap, batch=5, tile_fn=_stub_tile_fn(calls), blend_fn=_fp64_blend_fn, report=rep)
    assert out.shape == img.shape and out.dtype == np.uint8
    assert np.abs(out.astype(int) - img.astype(int)).max() <= 1              # exp(log(x)) and the truncation: within one level
    assert tuple(rep["tiles"]) == grid and rep["nonfinite"] == 0 and rep["bf16_rerun"] is False
    n = grid[0] * grid[1]
    assert sum(c[0][0] for c in calls) == n and all(c[0][0] <= 5 and c[0][1:] == (3,) + tuple(rep["tile_shape"]) for c in calls)
    with pytest.raises(ValueError):
        enhance.enhance_tiled(img, tile=tile, overlap=overlap, tile_fn=_stub_tile_fn([]))      # one injection point without the other


def test_host_gather_is_the_padded_image():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (21, 37, 3), dtype=np.uint8)
    p = harness.auto_padding(21, 37)
    whole = harness.tile_gather(img, [(-p[0], -p[2])], 21 + p[0] + p[1], 37 + p[2] + p[3])
    assert np.array_equal(whole.numpy(), harness.preprocess_unpaired(img).numpy())
    far = harness.tile_gather(img[:3, :5], [(-9, -11)], 25, 22)                  # pads longer than the image
    assert np.array_equal(far.numpy(), harness.preprocess_unpaired(img[:3, :5], (9, 13, 11, 6)).numpy())


def test_enhance_tiled_reruns_a_nonfinite_image_in_bf16():
    img = np.full((40, 70, 3), 9, np.uint8)
    calls = []

    def tile_fn(lr, precision):
        calls.append(precision)
        out = np.full(lr.shape, 0.5 if precision == "bf16" else 0.25, np.float32)
        if precision != "bf16":
            out[0, 0, 0, 0] = np.inf
        return out

    rep = {}
    out = enhance.enhance_tiled(img, tile=32, overlap=16, batch=64, tile_fn=tile_fn, blend_fn=_fp64_blend_fn, report=rep)
    assert calls == [None, "bf16"] and rep["bf16_rerun"] is True and rep["nonfinite"] == 0
    assert (out == 127).all()


def test_enhance_images_tiles_only_with_tile_and_only_large_images():
    small, big = np.full((10, 12, 3), 40, np.uint8), np.full((40, 70, 3), 80, np.uint8)
    untiled = []

    def enhance_fn(batch_u8, pads, precision):
        a = np.asarray(batch_u8)
        untiled.append(a.shape)
        return 255 - a, np.zeros(a.shape[0], np.int32)

    rep = {}
    outs = enhance.enhance_images([small, big], enhance_fn=enhance_fn, names=["s.png", "b.png"], report=rep, tile=32, overlap=16,
                                  tile_fn=_stub_tile_fn([]), blend_fn=_fp64_blend_fn)
    assert untiled == [(1, 10, 12, 3)] and (outs[0] == 215).all()             # the small image: today's path
    assert outs[1].shape == big.shape and np.abs(outs[1].astype(int) - 80).max() <= 1
    assert rep["tiles"] == {"b.png": [2, 4]} and rep["padded"] == [[16, 16], [32, 32]] and rep["bf16_rerun_images"] == []
    # without `tile` nothing changes: the oversize image is refused before any launch
    calls = []
    with pytest.raises(ValueError, match="big.png"):
        enhance.enhance_images([small, np.zeros((2200, 3900, 3), np.uint8)], enhance_fn=lambda *a: calls.append(a), names=["ok.png", "big.png"])
    assert calls == []


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """Host-side argument checks of the two entry points (nothing is launched: every call below fails a check first)."""
    from glare_amd import _lib

    lib = _lib.main_lib()
    p = 4096                                                   # a non-NULL, 16-byte aligned stand-in for a device pointer
    S, R = harness.PAD_SYMMETRIC, harness.PAD_REFLECT101
    for args in ((None, 4, 4, p, 1, 8, 8, S, p), (p, 4, 4, None, 1, 8, 8, S, p), (p, 4, 4, p, 1, 8, 8, S, None), (p, 0, 4, p, 1, 8, 8, S, p),
                 (p, 4, 4, p, 0, 8, 8, R, p), (p, 4, 4, p, 1, 0, 8, R, p), (p, 4, 4, p, 1, 8, -8, R, p), (p, 4, 4, p, 1, 8, 8, 2, p),
                 (p, 4, 4, p, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, S, p)):
        assert lib.glare_harness_tile_gather_u8(*args, None) == _lib.ERR_INVALID, args
    nws = lib.glare_harness_tile_blend_workspace_bytes()
    assert 0 < nws <= 1 << 16
    good = [p, 2, 2, 32, 32, p, p, 40, 40, p, p, p, p, p, p, p, p, nws]
    for i, v in ((0, None), (1, 0), (2, -1), (3, 0), (4, 0), (5, None), (6, None), (7, 0), (8, 0), (9, None), (10, None), (11, None),
                 (12, None), (13, None), (13, p + 2), (14, p + 4)):
        args = list(good)
        args[i] = v
        assert lib.glare_harness_tile_blend_f32(*args, None) == _lib.ERR_INVALID, (i, v)
    for i, v in ((16, None), (17, nws - 1)):                   # the count needs the workspace
        args = list(good)
        args[i] = v
        assert lib.glare_harness_tile_blend_f32(*args, None) == _lib.ERR_WORKSPACE, (i, v)


def test_tile_kernels_build_for_gfx950_without_scratch():
    """The two kernels (and the count's final sum) compile for gfx950 with 0 B of scratch per lane, in both libraries' builds."""
    import os
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    sys.path.insert(0, os.path.join(root, "glare_amd", "csrc"))
    import build as B

    for half in (False, True):
        cmd = [hipcc] + [f for f in B.COMMON if f != "-fPIC"] + (["-DGLARE_ACT_F16"] if half else []) + [
            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(root, "glare_amd", "csrc", "harness.hip"), "-o", os.devnull]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        names = re.findall(r"Function Name: (\S+)", r.stderr)
        scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
        assert len(names) == len(scratch)
        mine = {n: s for n, s in zip(names, scratch) if "tile_" in n}
        assert len(mine) == 3 and any("tile_gather_kernel" in n for n in mine) and any("tile_blend_kernel" in n for n in mine), mine
        assert all(s == 0 for s in mine.values()), mine
