"""GPU: `python -m glare_amd.evaluate stage1` end to end on a synthetic folder (three 32 x 48 pairs, two `*_VQ.pth` files whose codebooks
lie on the encoder's latents, so that more than one code is in use) -- every file it writes, each image's `codes` and the split's
`codebook` block against tests/usage_fp64.py applied to decode_nhwc's own indices, the mean PSNR against fit.make_validate_stage1 to the
last bit -- and Stage1Trainer(codebook_usage=True): the two logged terms against the restatement, and a default trainer left as it was."""
import csv
import json
import os
import types

import numpy as np
import pytest
import torch

import usage_fp64 as U
from glare_amd import checkpoint, data, evaluate, fit, harness
from glare_amd import modules as M
from glare_amd.synthetic import seeded_init_, synthetic_pair
from glare_amd.train import Stage1Trainer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 8192
H, W = 32, 48
NAMES = ["00.png", "01.png", "02.png"]


def _prior(seed):
    """A name-seeded VQModel whose codebook is 8192 of its own encoder's latents (synthetic.representative_init_, step 1)."""
    net = seeded_init_(M.VQModel().eval(), seed).to(DEV)
    _, normal = synthetic_pair(4, 192, 192, seed=seed * 31 + 7)
    x = torch.from_numpy(normal).permute(0, 3, 1, 2).float().div(255).to(DEV)
    with torch.no_grad():
        tokens = net.encode_nhwc(x).reshape(-1, 3)
        assert tokens.shape[0] >= K
        pick = torch.randperm(tokens.shape[0], generator=torch.Generator().manual_seed(seed + 5))[:K]
        net.quantize.embedding.weight.copy_(tokens[pick.to(DEV)])
    net.invalidate()
    return net


@pytest.fixture(scope="module")
def swept(tmp_path_factory):
    """The folder, the run and ONE sweep of it (--batch 1 --save-images), shared by the tests below."""
    from PIL import Image

    tmp = tmp_path_factory.mktemp("stage1")
    root, run = str(tmp / "data"), str(tmp / "run")
    lows, highs = synthetic_pair(3, H, W, seed=9)
    for sub, imgs in (("low", lows), ("high", highs)):
        os.makedirs(os.path.join(root, "eval15", sub))
        for nm, im in zip(NAMES, imgs):
            Image.fromarray(im).save(os.path.join(root, "eval15", sub, nm))
    os.makedirs(os.path.join(run, "models"))
    for it, seed in ((2, 1), (10, 4)):
        checkpoint.save_network(_prior(seed), os.path.join(run, "models", "%d_VQ.pth" % it))
    res = evaluate.main(["stage1", "--run", run, "--root", root, "--batch", "1", "--save-images"])
    pairs = data.LAYOUTS["v1"]({"root": root}, train=False).pairs            # rows are written in the dataset's order
    assert sorted(p[2] + ".png" for p in pairs) == NAMES
    return types.SimpleNamespace(root=root, run=run, out=os.path.join(run, "results-stage1"), res=res, names=[p[2] + ".png" for p in pairs],
                                 highs=np.stack([p[1] for p in pairs]))


def _loaded(run, name):
    net = M.VQModel().eval().to(DEV)
    evaluate.load_checkpoint(os.path.join(run, "models", name + ".pth"), net)
    return net


def _assert_block(block, counts_row):
    want = U.stats(counts_row)
    assert set(block) == {"tokens", "active", "active_fraction", "perplexity"}
    assert block["tokens"] == want["tokens"] and block["active"] == want["active"] and block["active_fraction"] == want["active"] / K
    assert abs(block["perplexity"] - want["perplexity"]) <= U.perplexity_bound(K, want["abs_terms"]) * want["perplexity"]


def test_files_of_the_sweep_and_the_usage_against_the_restatement(swept):
    res, out = swept.res, swept.out
    assert res["stage"] == "stage1" and res["images"] == 3 and res["select"] == "PSNR"
    assert [c["name"] for c in res["checkpoints"]] == ["2_VQ", "10_VQ"] and not any(c["skipped"] for c in res["checkpoints"])
    assert list(res["codebook"]) == ["2_VQ", "10_VQ"] and json.loads(json.dumps(res)) == res
    assert res["best"]["column"] == "PSNR" and res["best"]["name"] in ("2_VQ", "10_VQ")
    lines = open(os.path.join(out, "results-stage1.txt")).read().splitlines()
    assert [l.split(" ", 1)[0] for l in lines] == ["2_VQ", "10_VQ"]
    for rec, line in zip(res["checkpoints"], lines):
        name = rec["name"]
        with open(os.path.join(out, name + ".csv"), newline="") as f:
            rows = list(csv.DictReader(f))
        assert list(rows[0]) == ["conf", "name", "PSNR", "SSIM", "codes"] and [r["name"] for r in rows] == swept.names
        assert rec["means"]["PSNR"] == float(np.mean([float(r["PSNR"]) for r in rows]))
        assert all(np.isfinite(float(r["PSNR"])) and 0 < float(r["PSNR"]) < 100 and -1 <= float(r["SSIM"]) <= 1 for r in rows)
        # decode_nhwc's own indices of a fresh instance with the file's weights, one image at a time as --batch 1
        net = _loaded(swept.run, name)
        total = np.zeros(K, np.int64)
        for j, row in enumerate(rows):
            with torch.no_grad():
                _, gt, u8, sse, idx = evaluate.stage1_reconstruct(net, swept.highs[j:j + 1])
            idx = idx.cpu().numpy()
            assert idx.size == (H // 4) * (W // 4) and idx.min() >= 0 and idx.max() < K
            c, oor = U.counts(idx, K)
            assert oor[0] == 0 and float(row["codes"]) == U.stats(c[0])["active"]
            total += c[0]
            assert float(row["PSNR"]) == harness.psnr_u8(int(sse[0]), 3 * H * W)
            ssim = harness.ssim_device(u8.float() / 255, gt)
            assert float(row["SSIM"]) == float(ssim[0])
            from PIL import Image

            assert np.array_equal(np.asarray(Image.open(os.path.join(out, name, swept.names[j]))), u8[0].cpu().numpy())
        saved = np.load(os.path.join(out, name + ".codes.npy"))
        assert saved.dtype == np.int64 and saved.shape == (K,) and np.array_equal(saved, total)
        assert U.stats(total)["active"] > 1                      # more than one code in use: the case is not degenerate
        _assert_block(rec["codebook"], total)
        assert res["codebook"][name] == rec["codebook"]
        b = rec["codebook"]
        assert line.endswith("codes: %0.4f, codebook_tokens: %d, codebook_active: %d, codebook_active_fraction: %0.4f, codebook_perplexity: %0.4f"
                             % (rec["means"]["codes"], b["tokens"], b["active"], b["active_fraction"], b["perplexity"]))
        print(name, rec["means"], b)


def test_mean_psnr_equals_the_training_drivers_validation_bit_for_bit(swept):
    test_ds = data.LAYOUTS["v1"]({"root": swept.root}, train=False)
    assert len(test_ds.pairs) == 3
    for rec in swept.res["checkpoints"]:
        net = _loaded(swept.run, rec["name"])
        val = fit.make_validate_stage1(types.SimpleNamespace(netG=net), test_ds, None)(0)
        assert val == {"images": 3, "psnr": rec["means"]["PSNR"]}
        # a trainer with the flag: the same split, the same kernels, the same block
        val = fit.make_validate_stage1(types.SimpleNamespace(netG=net, codebook_usage=True), test_ds, None)(0)
        assert val["psnr"] == rec["means"]["PSNR"] and val["codebook"] == rec["codebook"]
        assert not net.training


def test_resumed_sweep_scores_nothing_again_and_reads_the_counts_back(swept):
    res = evaluate.main(["stage1", "--run", swept.run, "--root", swept.root, "--batch", "1", "--select", "codes"])
    assert [c["skipped"] for c in res["checkpoints"]] == [True, True] and res["best"]["column"] == "codes"
    for a, b in zip(res["checkpoints"], swept.res["checkpoints"]):
        assert a["means"] == b["means"] and a["codebook"]["tokens"] == b["codebook"]["tokens"] and a["codebook"]["active"] == b["codebook"]["active"]
        assert a["codebook"]["perplexity"] == pytest.approx(b["codebook"]["perplexity"], rel=1e-12)      # numpy's fp64 and the kernel's
    assert res["best"]["value"] == max(c["means"]["codes"] for c in res["checkpoints"])


def test_a_batch_of_padded_images_counts_each_image_on_its_own():
    """30 x 45 pads to 32 x 48; three images in one batch = three groups of one launch."""
    net = _prior(4)
    _, highs = synthetic_pair(3, 30, 45, seed=3)
    with torch.no_grad():
        img, _, u8, _, idx = evaluate.stage1_reconstruct(net, highs)
    assert tuple(img.shape) == (3, 3, 32, 48) and tuple(u8.shape) == (3, 30, 45, 3) and idx.numel() == 3 * 8 * 12
    counts, oor = U.counts(idx.cpu().numpy(), K, groups=3)
    report = {}
    rows = evaluate.score_checkpoint("stage1", net, None, highs, highs, batch=3, report=report)
    assert [r["codes"] for r in rows] == [float(U.stats(c)["active"]) for c in counts] and tuple(rows[0]) == ("PSNR", "SSIM", "codes")
    assert np.array_equal(report["codes"], counts.sum(0)) and report["codebook"]["out_of_range"] == 0 and report["bf16_rerun_images"] == []
    _assert_block({k: report["codebook"][k] for k in evaluate.USAGE_KEYS}, counts.sum(0))


def _trainer(**kw):
    tr = Stage1Trainer(seeded_init_(M.VQModel().train(), 6).to(DEV), precision="fp16", **kw)
    tr.opt.scale.fill_(1024.0)          # as tests/test_gpu_stage1.py: a scale no step of this toy problem overflows at
    return tr


def _batch(seed=31, B=2, S=64):
    return torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _assert_terms(tr):
    idx = tr.net.last_indices.cpu().numpy()
    want = U.stats(U.counts(idx, K)[0][0])
    act, per = tr.last_terms["codebook_active"], tr.last_terms["codebook_perplexity"]
    assert act.is_cuda and per.is_cuda and act.dtype == torch.int64 and per.dtype == torch.float64 and act.dim() == per.dim() == 0
    assert int(act) == want["active"]
    assert abs(float(per) - want["perplexity"]) <= U.perplexity_bound(K, want["abs_terms"]) * want["perplexity"]
    return want


def test_trainer_with_the_flag_logs_usage_and_the_default_trainer_is_unchanged():
    x = _batch()
    plain, off, on = _trainer(), _trainer(codebook_usage=False), _trainer(codebook_usage=True)
    assert plain.log_terms() == off.log_terms() == () and on.log_terms() == ("codebook_active", "codebook_perplexity")
    losses = {"plain": [], "off": [], "on": []}
    for _ in range(4):
        for name, tr in (("plain", plain), ("off", off), ("on", on)):
            losses[name].append(tr.step_tensor(x).clone())
        assert set(plain.last_terms) == set(off.last_terms) == {"l1_loss", "codebook_loss"}
        assert set(on.last_terms) == {"l1_loss", "codebook_loss", "codebook_active", "codebook_perplexity"}
        want = _assert_terms(on)
    print("last step:", want)
    for a, b, c in zip(losses["plain"], losses["off"], losses["on"]):            # bit for bit: counting reads the indices, nothing else
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    for tr in (off, on):
        assert torch.equal(plain.opt.groups[0].w, tr.opt.groups[0].w) and torch.equal(plain.opt.groups[0].m, tr.opt.groups[0].m)
    assert "codebook_usage" not in plain.extra_state() and on.extra_state() == {}         # usage is not state


def test_gan_step_with_the_flag_logs_usage_too():
    torch.manual_seed(3)
    disc = M.NLayerDiscriminator().to(DEV)
    tr = _trainer(codebook_usage=True, discriminator=disc, disc_start=1)
    tr.opt_d.scale.fill_(1024.0)
    x = _batch(33)
    tr.step_tensor(x)                                                    # before disc_start: the plain step
    assert set(tr.last_terms) == {"l1_loss", "codebook_loss", "g_loss", "d_weight", "d_loss", "codebook_active", "codebook_perplexity"}
    _assert_terms(tr)
    tr.step_tensor(x)                                                    # the GAN step
    assert set(tr.last_terms) == {"l1_loss", "codebook_loss", "g_loss", "d_weight", "d_loss", "codebook_active", "codebook_perplexity"}
    _assert_terms(tr)
    assert tr.log_terms() == ("g_loss", "d_weight", "d_loss", "codebook_active", "codebook_perplexity")
