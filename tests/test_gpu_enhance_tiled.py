"""GPU: tiled enhancement (glare_amd.enhance.enhance_tiled) end to end -- one window equals the untiled path byte for byte, a 2 x 2
grid equals four single runs blended in fp64, the CLI on a folder of mixed sizes, and a 4K UHD frame, which the untiled path refuses."""
import json

import numpy as np
import pytest
import torch

from glare_amd import enhance, harness, ops
from glare_amd.synthetic import synthetic_pair

import tile_fp64 as T64

pytestmark = pytest.mark.gpu

from test_gpu_precision import setup  # noqa: E402


def _nets():
    _, _, pg, pv, _, _ = setup("representative", 36, 28, 33)      # trained-like weights (shared with test_gpu_enhance.py)
    return pg, pv


@pytest.mark.parametrize("h,w", [(40, 60), (64, 64)])
def test_single_tile_equals_untiled(h, w):
    pg, pv = _nets()
    img = synthetic_pair(1, h, w, seed=111)[0][0]
    rep = {}
    tiled = enhance.enhance_tiled(img, pg, pv, tile=64, overlap=16, report=rep)
    plain = enhance.enhance_images([img], pg, pv)[0]
    p = harness.auto_padding(h, w)
    assert rep["tiles"] == [1, 1] and rep["tile_shape"] == [h + p[0] + p[1], w + p[2] + p[3]] and rep["nonfinite"] == 0
    assert tiled.shape == img.shape and tiled.dtype == np.uint8
    assert np.array_equal(tiled, plain)


def test_2x2_tiles_equal_four_single_runs_blended_in_fp64(capsys):
    pg, pv = _nets()
    h, w, tile, overlap = 96, 112, 64, 16
    img = synthetic_pair(1, h, w, seed=112)[0][0]
    plan = enhance.plan_tiles(h, w, tile, overlap)
    assert plan["ys"] == [0, 32] and plan["xs"] == [0, 48] and (plan["th"], plan["tw"]) == (64, 64)
    origins = [(y, x) for y in plan["ys"] for x in plan["xs"]]
    img_d = torch.from_numpy(img).cuda()
    ops.ATTENTION_KEY_SPLITS_OVERRIDE = 1          # B = 1 and B = 4 otherwise split the keys differently (summation order)
    try:
        singles = []
        for o in origins:
            lr = harness.tile_gather_device(img_d, torch.tensor([o], dtype=torch.int32).cuda(), 64, 64)
            with torch.no_grad():
                singles.append(pg.reverse_flow_nhwc(pv, lr)["out"].float().cpu())
        rep = {}
        tiled = enhance.enhance_tiled(img, pg, pv, tile=tile, overlap=overlap, batch=4, report=rep)
    finally:
        ops.ATTENTION_KEY_SPLITS_OVERRIDE = None
    outs = torch.cat(singles).numpy()
    assert outs.shape == (4, 3, 64, 64) and np.isfinite(outs).all()
    acc, bad = T64.blend64(outs, plan["ys"], plan["xs"], h, w, 64, 64, overlap)
    wrong, share = T64.u8_mismatch(tiled, acc)
    with capsys.disabled():
        print("\n[2x2 tiles 96x112] uint8 values off the fp64 blend of four single runs: %d; off by one at a step: %.4f %% (cap 0.5)"
              % (wrong, 100 * share))
    assert rep["tiles"] == [2, 2] and rep["nonfinite"] == bad == 0 and rep["bf16_rerun"] is False
    assert tiled.shape == img.shape
    assert wrong == 0
    assert share <= T64.U8_CAP


def test_cli_on_a_folder_of_mixed_sizes_with_tile(tmp_path, capsys):
    from PIL import Image

    src, out, out_plain = tmp_path / "photos", tmp_path / "out", tmp_path / "plain"
    src.mkdir()
    sizes = {"small.png": (40, 60), "large.png": (100, 130)}
    for i, (n, (h, w)) in enumerate(sizes.items()):
        Image.fromarray(synthetic_pair(1, h, w, seed=120 + i)[0][0]).save(src / n)
    res = enhance.main([str(src), "--out", str(out), "--tile", "64", "--tile-overlap", "16"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    by_name = {r["name"]: r for r in line["images"]}
    assert set(by_name) == set(sizes) and line["skipped"] == [] and line["bf16_rerun_images"] == []
    assert by_name["large.png"]["tiles"] == [2, 3] and "tiles" not in by_name["small.png"]
    assert [r.get("tiles") for r in res["images"]] == [r.get("tiles") for r in line["images"]]
    for n, (h, w) in sizes.items():
        assert np.asarray(Image.open(out / n)).shape == (h, w, 3)
    enhance.main([str(src / "small.png"), "--out", str(out_plain)])
    capsys.readouterr()
    assert np.array_equal(np.asarray(Image.open(out / "small.png")), np.asarray(Image.open(out_plain / "small.png")))


def test_uhd_image_in_512_tiles_is_finite_and_repeatable(capsys):
    import time

    pg, pv = _nets()
    img = synthetic_pair(1, 2160, 3840, seed=131)[0][0]           # the dark half of the pair
    with pytest.raises(ValueError):
        enhance.enhance_images([img], pg, pv)                    # untiled: outside the envelope, refused before any launch
    rep = {}
    t0 = time.perf_counter()
    a = enhance.enhance_tiled(img, pg, pv, tile=512, report=rep)
    t1 = time.perf_counter()
    b = enhance.enhance_tiled(img, pg, pv, tile=512)
    t2 = time.perf_counter()
    with capsys.disabled():
        print("\n[UHD 2160x3840, tile 512, overlap 64] %d x %d tiles: first run %.2f s, second %.2f s (%.2f MP/s)"
              % (rep["tiles"][0], rep["tiles"][1], t1 - t0, t2 - t1, 2160 * 3840 / 1e6 / (t2 - t1)))
    assert rep["tiles"] == [5, 9] and rep["nonfinite"] == 0 and rep["bf16_rerun"] is False
    assert a.shape == img.shape and a.dtype == np.uint8
    assert np.array_equal(a, b)
