"""CPU: the host side of `glare_amd.evaluate stage1` -- the sweep's mechanics over a stage-1 run's `*_VQ.pth` files with stub networks and an
injected score function (as tests/test_evaluate_host.py does for stages 2 and 3) -- and the `--codebook-usage` switch of glare_amd.fit."""
import csv
import json
import os

import numpy as np
import pytest

import usage_fp64 as U
from glare_amd import evaluate, fit

K = 16


class _Net:
    weights = None


def _codes(it):
    """The split's histogram a stub checkpoint reports: `it` tokens on code 0, one on each of the next it % 5 + 1 codes."""
    c = np.zeros(K, np.int64)
    c[0] = it
    c[1:2 + it % 5] = 1
    return c


def _stub_sweep(tmp_path, files, select="PSNR", with_block=False, **kw):
    calls = []

    def load_fn(path, net):
        net.weights = path

    def score_fn(stage_, netG, net_hq, lows, gts, report=None, **unused):
        it = int(os.path.basename(netG.weights).split("_")[0])
        calls.append(it)
        report["bf16_rerun_images"] = []
        report["codes"] = _codes(it)
        if with_block:                                 # what score_checkpoint adds from the device's statistics
            report["codebook"] = {"tokens": 1, "active": 1, "active_fraction": 1 / K, "perplexity": 1.0, "out_of_range": 0}
        val = {2: 18.0, 10: 21.5, 30: 20.0}[it]
        # PSNR best at 10, codes best at 30
        return [{"PSNR": val + j, "SSIM": val / 100, "codes": float(it + j)} for j in range(len(lows))]

    lows = gts = np.zeros((3, 4, 4, 3), np.uint8)
    res = evaluate.sweep("stage1", files, str(tmp_path / "out"), lows, gts, names=["a.png", "b.png", "c.png"], nets=(_Net(), None),
                         select=select, score_fn=score_fn, load_fn=load_fn, warm_fn=lambda *a: None, **kw)
    return res, calls


def _models(tmp_path, names=("10_VQ.pth", "2_VQ.pth", "30_VQ.pth", "30_D.pth", "5_G.pth")):
    d = tmp_path / "run" / "models"
    d.mkdir(parents=True)
    for n in names:
        (d / n).write_bytes(b"")
    return str(tmp_path / "run")


def test_columns_and_the_vq_listing():
    assert evaluate.columns("stage1") == ("PSNR", "SSIM", "codes")
    assert evaluate.columns("stage1", True) == ("PSNR", "SSIM", "codes", "LPIPS")
    assert evaluate.stage1_pads(400, 600) == (0, 0, 0, 0) and evaluate.stage1_pads(33, 47) == (0, 3, 0, 1)


def test_sweep_lists_vq_files_writes_csv_codebook_and_codes(tmp_path):
    run = _models(tmp_path)
    assert [os.path.basename(f) for f in evaluate.list_checkpoints(run, "stage1")] == ["2_VQ.pth", "10_VQ.pth", "30_VQ.pth"]
    assert [os.path.basename(f) for f in evaluate.list_checkpoints(run)] == ["5_G.pth"]                  # the later stages: *_G only
    res, calls = _stub_sweep(tmp_path, run)
    assert calls == [2, 10, 30]
    out = tmp_path / "out"
    with open(out / "10_VQ.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0]) == ["conf", "name", "PSNR", "SSIM", "codes"]
    assert [r["name"] for r in rows] == ["a.png", "b.png", "c.png"] and rows[0]["conf"] == "train_stage1_LOL"
    assert [float(r["PSNR"]) for r in rows] == [21.5, 22.5, 23.5] and [float(r["codes"]) for r in rows] == [10.0, 11.0, 12.0]
    for it in (2, 10, 30):
        saved = np.load(out / ("%d_VQ.codes.npy" % it))
        assert saved.dtype == np.int64 and np.array_equal(saved, _codes(it))
    want = U.stats(_codes(10))
    block = res["checkpoints"][1]["codebook"]
    assert set(block) == {"tokens", "active", "active_fraction", "perplexity"}
    assert block["tokens"] == want["tokens"] == 11 and block["active"] == want["active"] == 2 and block["active_fraction"] == 2 / K
    assert block["perplexity"] == pytest.approx(want["perplexity"], rel=1e-12)
    assert res["codebook"] == {c["name"]: c["codebook"] for c in res["checkpoints"]} and list(res["codebook"]) == ["2_VQ", "10_VQ", "30_VQ"]
    lines = open(out / "results-stage1.txt").read().splitlines()
    assert [l.split(" ", 1)[0] for l in lines] == ["2_VQ", "10_VQ", "30_VQ"]
    assert lines[1] == ("10_VQ PSNR: 22.5000, SSIM: 0.2150, codes: 11.0000, codebook_tokens: 11, codebook_active: 2, "
                        "codebook_active_fraction: 0.1250, codebook_perplexity: %0.4f" % want["perplexity"])
    assert res["best"] == {"name": "10_VQ", "column": "PSNR", "value": 22.5} and res["stage"] == "stage1"
    assert json.loads(json.dumps(res)) == res
    assert not [f for f in os.listdir(out) if f.endswith("_")]


def test_sweep_keeps_the_device_block_without_out_of_range(tmp_path):
    res, _ = _stub_sweep(tmp_path, _models(tmp_path), with_block=True)
    assert res["checkpoints"][0]["codebook"] == {"tokens": 1, "active": 1, "active_fraction": 1 / K, "perplexity": 1.0}


def test_resumed_sweep_skips_and_reads_the_usage_back(tmp_path):
    run = _models(tmp_path)
    res, calls = _stub_sweep(tmp_path, run)
    os.remove(tmp_path / "out" / "30_VQ.csv")
    res2, calls2 = _stub_sweep(tmp_path, run, select="codes")
    assert calls == [2, 10, 30] and calls2 == [30]
    assert [c["skipped"] for c in res2["checkpoints"]] == [True, True, False]
    assert res2["checkpoints"][1]["codebook"] == res["checkpoints"][1]["codebook"]          # from 10_VQ.codes.npy
    assert res2["codebook"] == res["codebook"]
    assert res2["best"] == {"name": "30_VQ", "column": "codes", "value": 31.0}             # --select codes: higher is better


def test_select_of_a_foreign_column_raises_before_anything_is_scored(tmp_path):
    run = _models(tmp_path)
    for col in ("1_PSNR", "Adjust_PSNR", "LPIPS", "perplexity"):          # LPIPS: not without a LPIPS net
        with pytest.raises(ValueError):
            _, calls = _stub_sweep(tmp_path, run, select=col)
    assert not os.path.exists(tmp_path / "out")
    res, calls = _stub_sweep(tmp_path, run, select="SSIM")
    assert calls == [2, 10, 30] and res["best"]["name"] == "10_VQ"


def test_net_vq_is_refused_for_stage1(tmp_path, capsys):
    with pytest.raises(ValueError, match="run's own"):
        evaluate.build_nets("stage1", net_vq=str(tmp_path / "prior.pth"))
    with pytest.raises(SystemExit):
        evaluate.main(["stage1", "--run", str(tmp_path), "--root", str(tmp_path), "--net-vq", str(tmp_path / "prior.pth")])
    assert "run's own" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                       # a foreign --select, refused by the command as well
        evaluate.main(["stage1", "--run", str(tmp_path), "--root", str(tmp_path), "--select", "1_PSNR"])
    assert "stage1 produces PSNR, SSIM, codes" in capsys.readouterr().err


def test_fit_takes_codebook_usage_for_stage1_only(tmp_path, capsys):
    base = ["--root", str(tmp_path), "--out", str(tmp_path / "run")]
    args, _ = fit.parse_args(["stage1"] + base + ["--codebook-usage"])
    assert args.codebook_usage is True
    assert fit.parse_args(["stage1"] + base)[0].codebook_usage is False
    for stage in ("stage2", "stage3"):
        with pytest.raises(SystemExit):
            fit.parse_args([stage] + base + ["--codebook-usage"])
        assert "--codebook-usage is a stage1 option" in capsys.readouterr().err
        with pytest.raises(ValueError, match="stage1 option"):
            fit.build_trainer(stage, fit.default_options(stage), None, codebook_usage=True)
