"""CPU: the host side of the checkpoint sweep (glare_amd.evaluate; code/test_stage2.py, code/test_stage3.py) -- the numpy
restatements of the "adjust" protocol that the GPU tests use as their oracle, and the sweep's mechanics with stub networks and an
injected score function."""
import csv
import ctypes
import json
import math
import os

import numpy as np
import pytest

from glare_amd import _lib, evaluate, harness


def _gt(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def test_score_u8_truncates_at_the_k_over_255_boundaries():
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    x = np.stack([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2))])          # [3, 256]: below, on, above k/255
    out = np.broadcast_to(x[None, None], (1, 3, 3, 256)).copy()                                   # [B=1][3][h=3][w=256]
    u8, sse = harness.score_u8(out, np.zeros((1, 3, 256, 3), np.uint8))
    want = (np.clip(x.astype(np.float64), 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)   # rgb(): fp32 product, truncated
    assert np.array_equal(u8[0, :, :, 0], want) and np.array_equal(u8[0, :, :, 1], want)
    assert np.all(u8[0, 0, 1:, 0] <= np.arange(1, 256)) and np.all(u8[0, 0, 1:, 0] >= np.arange(1, 256) - 1)   # just below k/255: k or k - 1
    assert int(sse[0]) == 3 * int((want.astype(np.int64) ** 2).sum())
    # truncation, not rounding: 0.999 * 255 = 254.7 -> 254 (img_as_ubyte would give 255)
    assert harness.score_u8(np.full((1, 3, 1, 1), 0.999, np.float32), np.zeros((1, 1, 1, 3), np.uint8))[0].ravel().tolist() == [254] * 3


def test_score_u8_special_values_and_the_gain():
    out = np.array([np.nan, np.inf, -np.inf, -0.5, 1.5, 0.5], np.float32).reshape(1, 3, 1, 2)    # planes: (nan, inf) (-inf, -.5) (1.5, .5)
    gt = np.zeros((1, 1, 2, 3), np.uint8)
    u8, sse = harness.score_u8(out, gt)
    assert u8.tolist() == [[[[0, 0, 255], [255, 0, 127]]]]            # NaN -> 0, +inf -> 255, HWC order
    assert int(sse[0]) == 2 * 255 ** 2 + 127 ** 2
    u8g, _ = harness.score_u8(out, gt, gain=np.array([0.5], np.float32))
    assert u8g.tolist() == [[[[0, 0, 191], [255, 0, 63]]]]            # 1.5 * .5 = .75 -> 191; .25 -> 63
    u8z, _ = harness.score_u8(out, gt, gain=np.array([0.0], np.float32))
    assert not u8z.any()                                               # inf * 0 = NaN -> 0
    # the window
    big = np.zeros((2, 3, 5, 6), np.float32)
    big[:, :, 1:3, 2:5] = 1.0
    u8w, ssew = harness.score_u8(big, np.full((2, 2, 3, 3), 255, np.uint8), window=(1, 2, 2, 3))
    assert u8w.shape == (2, 2, 3, 3) and np.all(u8w == 255) and ssew.tolist() == [0, 0]


def test_adjust_gain_uses_raw_values_and_the_bgr2gray_weights():
    out = np.zeros((2, 3, 2, 2), np.float32)
    out[0] = [[[3.0, -1.0], [0.5, 0.5]]] * 3                  # raw mean 0.75; clamped first it would be (1 + 0 + .5 + .5) / 4 = 0.5
    out[1] = 0.25
    gt = np.zeros((2, 2, 2, 3), np.uint8)
    gt[0] = 255                                               # gray mean / 255 = 1
    gt[1, ..., 0], gt[1, ..., 1], gt[1, ..., 2] = 255, 0, 0   # 0.114 (the weight cv2's BGR2GRAY puts on channel 0 of RGB data)
    g = harness.adjust_gain(out, gt)
    assert g.dtype == np.float32
    assert g[0] == np.float32(1 / 0.75) and g[0] != np.float32(1 / 0.5)
    assert g[1] == np.float32(0.114 / 0.25)
    assert harness.adjust_gain(out, gt, window=(0, 0, 2, 2)).tolist() == g.tolist()
    assert abs(float(harness.adjust_gain(out[1:], gt[1:])[0]) - harness.gray_mean(gt[1] / 255) / 0.25) < 1e-6
    assert np.isnan(harness.adjust_gain(np.full((1, 3, 1, 1), np.nan, np.float32), gt[:1, :1, :1]))[0]


def test_psnr_u8_is_ten_log10_of_peak_squared_over_mse():
    rng = np.random.default_rng(3)
    a, b = _gt((7, 9, 3), 1), _gt((7, 9, 3), 2)
    out = (a.astype(np.float32) / 255).transpose(2, 0, 1)[None]
    u8, sse = harness.score_u8(out, b[None])
    mse = np.mean((u8[0].astype(np.float64) - b.astype(np.float64)) ** 2)
    assert harness.psnr_u8(sse[0], a.size) == pytest.approx(10 * np.log10(255.0 ** 2 / mse), rel=1e-14)
    assert harness.psnr_u8(65025 * 5, 5) == 0.0
    assert harness.psnr_u8(0, 100) == math.inf                # skimage returns inf for equal images
    assert harness.psnr_u8(np.int64(1), 1) == pytest.approx(48.1308036086791)
    del rng


def test_header_types_the_new_entries():
    sigs = _lib.signatures()
    c = ctypes
    assert sigs["glare_harness_score_workspace_bytes"] == (c.c_size_t, [c.c_int])
    assert sigs["glare_harness_adjust_gain_f32"] == (c.c_int, [c.c_void_p] * 2 + [c.c_int] * 7 + [c.c_void_p] * 2 + [c.c_size_t, c.c_void_p])
    assert sigs["glare_harness_score_u8"] == (c.c_int, [c.c_void_p] * 3 + [c.c_int] * 7 + [c.c_void_p] * 3 + [c.c_size_t, c.c_void_p])
    lib = _lib.lib()
    assert lib.glare_version() >= 122
    one = lib.glare_harness_score_workspace_bytes(1)
    assert one > 0 and lib.glare_harness_score_workspace_bytes(5) == 5 * one and lib.glare_harness_score_workspace_bytes(0) == 0
    # refused before anything is launched (no GPU here): null pointers, B = 0, a window outside the tensor
    assert lib.glare_harness_score_u8(None, None, None, 1, 8, 8, 0, 0, 8, 8, None, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.glare_harness_adjust_gain_f32(None, None, 1, 8, 8, 0, 0, 8, 8, None, None, 0, None) == _lib.ERR_INVALID


def test_stage2_pads_and_columns():
    assert evaluate.stage2_pads(400, 600) == (0, 0, 0, 0)
    assert evaluate.stage2_pads(43, 59) == (0, 1, 0, 1)
    for h, w in ((42, 60), (44, 57), (401, 600)):             # pad to even only, as the reference: 42 stays 42, not a multiple of 4
        with pytest.raises(ValueError):
            evaluate.stage2_pads(h, w)
    assert evaluate.columns("stage2") == ("Adjust_PSNR", "PSNR")
    assert evaluate.columns("stage2", True) == ("Adjust_PSNR", "Adjust_LPIPS", "PSNR", "LPIPS")
    assert evaluate.columns("stage3") == ("PSNR", "SSIM", "1_PSNR")
    assert evaluate.columns("stage3", True) == ("PSNR", "SSIM", "1_PSNR", "LPIPS")
    assert evaluate.format_measurements({"PSNR": 20.123456, "heat": 0}) == "PSNR: 20.1235, heat: 0"


class _Net:
    weights = None


def _stub_sweep(tmp_path, stage, files, select="PSNR", **kw):
    """The sweep with no device: load_fn records the file in the stub net, score_fn makes rows out of the checkpoint's number."""
    calls = []

    def load_fn(path, net):
        net.weights = path

    def score_fn(stage_, netG, net_hq, lows, gts, report=None, **unused):
        it = int(os.path.basename(netG.weights).split("_")[0])
        calls.append(it)
        report["bf16_rerun_images"] = [1] if it == 10 else []
        val = {2: 18.0, 10: 21.5, 30: 20.0}[it]
        return [{c: val + j + 0.25 * k for k, c in enumerate(evaluate.columns(stage_))} for j in range(len(lows))]

    lows = gts = np.zeros((3, 4, 4, 3), np.uint8)
    res = evaluate.sweep(stage, files, str(tmp_path / "out"), lows, gts, names=["a.png", "b.png", "c.png"], nets=(_Net(), _Net()),
                         select=select, score_fn=score_fn, load_fn=load_fn, warm_fn=lambda *a: None, **kw)
    return res, calls


def _models(tmp_path, names=("10_G.pth", "2_G.pth", "30_G.pth", "latest_D.pth")):
    d = tmp_path / "run" / "models"
    d.mkdir(parents=True)
    for n in names:
        (d / n).write_bytes(b"")
    return str(tmp_path / "run")


@pytest.mark.parametrize("stage", ["stage2", "stage3"])
def test_sweep_order_csv_results_and_best(tmp_path, stage):
    run = _models(tmp_path)
    assert [os.path.basename(f) for f in evaluate.list_checkpoints(run)] == ["2_G.pth", "10_G.pth", "30_G.pth"]     # natural order, *_G only
    res, calls = _stub_sweep(tmp_path, stage, run)
    assert calls == [2, 10, 30]
    cols = evaluate.columns(stage)
    out = tmp_path / "out"
    with open(out / "10_G.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    lead = ["conf", "heat", "name"] if stage == "stage2" else ["conf", "name"]
    assert list(rows[0]) == lead + list(cols)
    assert [r["name"] for r in rows] == ["a.png", "b.png", "c.png"] and rows[0]["conf"] == "train_%s_LOL" % stage
    assert [float(r[cols[0]]) for r in rows] == [21.5, 22.5, 23.5] and float(rows[2][cols[1]]) == 23.75
    lines = open(out / ("results-%s.txt" % stage)).read().splitlines()
    assert [l.split(" ", 1)[0] for l in lines] == ["2_G", "10_G", "30_G"]
    assert lines[1] == "10_G " + ", ".join("%s: %0.4f" % (c, 22.5 + 0.25 * k) for k, c in enumerate(cols))
    assert res["best"] == {"name": "10_G", "column": "PSNR", "value": 22.5 + 0.25 * cols.index("PSNR")}
    assert [c["name"] for c in res["checkpoints"]] == ["2_G", "10_G", "30_G"] and not any(c["skipped"] for c in res["checkpoints"])
    assert res["bf16_rerun_images"] == {"10_G": ["b.png"]}
    assert set(res["seconds_per_checkpoint"]) == {"load_repack", "scoring"} and res["images"] == 3
    assert json.loads(json.dumps(res)) == res
    assert not [f for f in os.listdir(out) if f.endswith("_")]           # no temporary CSV left


def test_sweep_skips_a_checkpoint_whose_csv_exists_and_still_ranks_it(tmp_path):
    run = _models(tmp_path)
    res, calls = _stub_sweep(tmp_path, "stage3", run)
    assert calls == [2, 10, 30]
    os.remove(tmp_path / "out" / "30_G.csv")
    res2, calls2 = _stub_sweep(tmp_path, "stage3", run, select="1_PSNR")
    assert calls2 == [30]                                                  # the reference resumes this way (test_stage2.py:126-127)
    assert [c["skipped"] for c in res2["checkpoints"]] == [True, True, False]
    assert res2["best"]["name"] == "10_G" and res2["best"]["value"] == pytest.approx(23.0)
    assert res2["checkpoints"][1]["means"] == res["checkpoints"][1]["means"]
    lines = open(tmp_path / "out" / "results-stage3.txt").read().splitlines()
    assert [l.split(" ", 1)[0] for l in lines] == ["2_G", "10_G", "30_G", "30_G"]     # appended, as the reference does


def test_sweep_takes_a_file_list_and_refuses_a_missing_column(tmp_path):
    run = _models(tmp_path)
    files = [os.path.join(run, "models", n) for n in ("30_G.pth", "2_G.pth")]
    res, calls = _stub_sweep(tmp_path, "stage2", files, select="Adjust_PSNR")
    assert calls == [2, 30] and res["best"]["name"] == "30_G" and res["best"]["column"] == "Adjust_PSNR"
    for stage, col in (("stage2", "SSIM"), ("stage3", "Adjust_PSNR"), ("stage3", "LPIPS")):      # LPIPS: not without a LPIPS net
        with pytest.raises(ValueError):
            _stub_sweep(tmp_path, stage, files, select=col)
    assert calls == [2, 30]


def test_score_checkpoint_refuses_sizes_before_any_launch():
    lows = np.zeros((1, 42, 60, 3), np.uint8)
    with pytest.raises(ValueError):                        # raised before the device is looked at: passes without a GPU
        evaluate.score_checkpoint("stage2", None, None, lows, lows)
    huge = np.zeros((1, 4000, 6000, 3), np.uint8)          # outside the kernels' size envelope (glare_amd.enhance.SIZE_TABLE)
    with pytest.raises(ValueError):
        evaluate.score_checkpoint("stage3", None, None, huge, huge)
