"""MI355X: the batch-assembly kernel (csrc/train_data.hip) behind glare_amd.data.DeviceLoLDataset against LoL_Dataset on the host,
bit for bit, and the training driver (glare_amd.fit) end to end on synthetic folders.

Step-1 loss of the driver against a hand-fed, identically seeded trainer (test_stage3_end_to_end): the inputs are bit-identical
(test_batch_equals_the_host_dataset), so the bound is the step's own run-to-run spread: the test steps two identically seeded hand-fed
trainers, takes |loss_a - loss_b| / |loss_a| as that spread and bounds the driver's step-1 loss at 2 x max(spread, 1e-6) relative from
the hand-fed one (eager and --graph alike); it prints all figures (-s).  Figures on an MI355X: NOT MEASURED YET -- this file has not
run on hardware; record the printed spread and the two distances here after the first GPU run."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from glare_amd import _lib, checkpoint, fit
from glare_amd import data as D

pytestmark = pytest.mark.gpu

SIZES = [(40, 56), (33, 47), (64, 48), (37, 37), (50, 50), (32, 61)]      # odd sizes, squares, one side equal to the crop


def _write(folder, name, h, w, rng):
    os.makedirs(folder, exist_ok=True)
    Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(folder, name))


def make_v1(root, split, sizes, seed=0):
    rng = np.random.default_rng(seed)
    for i, (h, w) in enumerate(sizes):
        _write(os.path.join(root, split, "low"), "%02d.png" % i, h, w, rng)
        _write(os.path.join(root, split, "high"), "%02d.png" % i, h, w, rng)


def _host_sample(ds, i, draw):
    low, high, _ = ds.pairs[i]
    lq = D.to_tensor(D.apply_augmentation(low, *draw))
    if ds.log_low:
        lq = torch.log(torch.clamp(lq + 1e-3, min=1e-3))
    return D.to_tensor(D.apply_augmentation(high, *draw)), lq


def _host_batch(ds, indices, draws):
    s = [_host_sample(ds, i, d) for i, d in zip(indices, draws)]
    return torch.stack([a for a, _ in s]), torch.stack([b for _, b in s])


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("small"))
    make_v1(root, "our485", SIZES)
    return root


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_batch_equals_the_host_dataset(small, precision):
    """7. torch.equal on GT and LQ: seeded draws (B = 1, B = 8, mixed sizes), every (flip, k) at the four corners, whole-image crops."""
    with _lib.use_precision(precision):
        for log_low in (True, False):
            ds = D.LoL_Dataset({"root": small, "use_crop": True, "use_flip": True, "use_rot": True, "GT_size": 32, "log_low": log_low}, train=True)
            dev = D.DeviceLoLDataset(ds, "cuda")
            for seed, idx in ((1, [3]), (2, [0, 1, 2, 3, 4, 5, 0, 3]), (3, [5, 4]), (4, [2, 2, 1, 0, 5, 4, 3, 1])):
                np.random.seed(seed)
                items = [ds[i] for i in idx]                                             # LoL_Dataset.__getitem__, collated
                gt_ref, lq_ref = torch.stack([s["GT"] for s in items]), torch.stack([s["LQ"] for s in items])
                np.random.seed(seed)
                gt, lq = dev.batch(idx)
                assert gt.shape == (len(idx), 3, 32, 32) and gt.dtype == torch.float32
                assert torch.equal(gt.cpu(), gt_ref) and torch.equal(lq.cpu(), lq_ref), (seed, idx, dev.last_draws)
            for flip in (0, 1):
                for k in (0, 1, 3):
                    idx = list(range(len(ds)))
                    for corner in range(4):                                              # crops touching all four borders
                        draws = [((h - 32) * (corner >> 1), (w - 32) * (corner & 1), 32, flip, k) for h, w in dev.hw]
                        gt, lq = dev.batch(idx, draws=draws)
                        gt_ref, lq_ref = _host_batch(ds, idx, draws)
                        assert torch.equal(gt.cpu(), gt_ref) and torch.equal(lq.cpu(), lq_ref), (flip, k, corner)
                    for i, (h, w) in enumerate(dev.hw):                                   # the crop is the whole image
                        if k and h != w:
                            continue
                        draws = [(0, 0, h if h == w else (h, w), flip, k)]
                        gt, lq = dev.batch([i], draws=draws)
                        gt_ref, lq_ref = _host_batch(ds, [i], draws)
                        assert gt.shape == (1, 3, h, w) and torch.equal(gt.cpu(), gt_ref) and torch.equal(lq.cpu(), lq_ref), (flip, k, i)


def test_invalid_rows_are_refused_before_any_launch(small):
    """8. GLARE_ERR_INVALID from the host side of the C entry, raised as the other ops raise."""
    ds = D.LoL_Dataset({"root": small, "use_crop": True, "GT_size": 32, "log_low": True}, train=True)
    dev = D.DeviceLoLDataset(ds, "cuda")
    h, w = dev.hw[0]
    bad = {"crop below the image": (h - 31, 0, 32, 0, 0), "crop right of the image": (0, w - 31, 32, 0, 0), "negative origin": (-1, 0, 32, 0, 0),
           "k = 2": (0, 0, 32, 0, 2), "flip = 2": (0, 0, 32, 2, 0), "non-square crop with rotation": (0, 0, (20, 30), 0, 1)}
    out = torch.full((1, 3, 32, 32), 7.0, device="cuda")
    for what, draw in bad.items():
        kw = {} if isinstance(draw[2], tuple) else {"out_gt": out}
        with pytest.raises(_lib.GlareError) as ei:
            dev.batch([0], draws=[draw], **kw)
        assert ei.value.status == _lib.ERR_INVALID and "glare_train_batch_u8" in str(ei.value), what
    with pytest.raises(_lib.GlareError):                    # a second sample whose crop size differs from the batch's
        dev.batch([0, 1], draws=[(0, 0, 32, 0, 0), (0, 0, 16, 0, 0)])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                         # nothing was launched
    with pytest.raises(ValueError):
        dev.update_captured([0], draws=[(0, 0, 32, 0, 2)])


def test_batch_writes_in_place_and_replays_with_a_new_table(small):
    """9. out_gt / out_lq are written in place; a captured batch() replayed after update_captured() yields the new batch."""
    ds = D.LoL_Dataset({"root": small, "use_crop": True, "use_flip": True, "use_rot": True, "GT_size": 32, "log_low": True}, train=True)
    dev = D.DeviceLoLDataset(ds, "cuda")
    gt, lq = torch.zeros(4, 3, 32, 32, device="cuda"), torch.zeros(4, 3, 32, 32, device="cuda")
    np.random.seed(5)
    a, b = dev.batch([0, 1, 2, 3], out_gt=gt, out_lq=lq)
    assert a is gt and b is lq
    first = dev.last_draws
    gt_ref, lq_ref = _host_batch(ds, [0, 1, 2, 3], first)
    assert torch.equal(gt.cpu(), gt_ref) and torch.equal(lq.cpu(), lq_ref)
    for _ in range(2 * dev.RING + 1):                                                        # the pinned ring wraps around
        dev.batch([3, 2, 1, 0], out_gt=gt, out_lq=lq)
    gt_ref, lq_ref = _host_batch(ds, [3, 2, 1, 0], dev.last_draws)
    assert torch.equal(gt.cpu(), gt_ref) and torch.equal(lq.cpu(), lq_ref)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.batch([0, 1, 2, 3], out_gt=gt, out_lq=lq, draws=first)
    for indices in ([0, 1, 2, 3], [5, 4, 4, 1], [2, 0, 5, 3]):
        if indices != [0, 1, 2, 3]:
            dev.update_captured(indices)
        gt.zero_(), lq.zero_()
        graph.replay()
        gt_ref, lq_ref = _host_batch(ds, indices, dev.last_draws)
        assert torch.equal(gt.cpu(), gt_ref) and torch.equal(lq.cpu(), lq_ref), indices


def _run(stage, root, out, tmp, *extra):
    opt = os.path.join(str(tmp), "opt.json")
    with open(opt, "w") as f:
        json.dump({"logger": {"print_freq": 1}}, f)
    return fit.main([stage, "--root", root, "--out", out, "--opt", opt] + list(extra))


def _hand_fed_step1(root):
    """The loss of step 1 of an identically seeded Stage3Trainer fed LoL_Dataset's host tensors for the driver's first indices."""
    options = fit.default_options("stage3")
    host = D.LoL_Dataset(dict(options["datasets"]["train"], root=root), train=True)
    tr = fit.build_trainer("stage3", options, torch.device("cuda", 0))
    tr.opt.betas = (options["train"]["beta1"], options["train"]["beta2"])
    fit.set_random_seed(options["train"]["manual_seed"])
    fit.make_schedule(tr.opt, options).update(1)
    indices = fit.epoch_batches(len(host), 2)[0]
    items = [host[i] for i in indices]
    gt, lq = torch.stack([s["GT"] for s in items]).cuda(), torch.stack([s["LQ"] for s in items]).cuda()
    return float(tr.step_tensor(gt, lq))


def test_stage3_end_to_end(tmp_path):
    """10. 6 synthetic pairs, niter 12, save every 6, name-seeded nets; eager and --graph; step-1 loss against the hand-fed trainer."""
    root = str(tmp_path / "data")
    make_v1(root, "our485", [(260, 300), (256, 256), (300, 270), (272, 401), (257, 263), (288, 256)], seed=1)
    make_v1(root, "eval15", [(44, 76)] * 3, seed=2)
    from glare_amd import modules as M

    hand_a, hand_b = _hand_fed_step1(root), _hand_fed_step1(root)
    spread = abs(hand_a - hand_b) / abs(hand_a)
    bound = 2 * max(spread, 1e-6)
    print("hand-fed step-1 loss %.9g / %.9g: run-to-run spread %.3g relative, bound %.3g" % (hand_a, hand_b, spread, bound))
    for graph in (False, True):
        out = str(tmp_path / ("run_graph" if graph else "run"))
        recs = _run("stage3", root, out, tmp_path, "--niter", "12", "--save-freq", "6", *(["--graph"] if graph else []))
        steps, summary = recs[:-1], recs[-1]
        assert [r["iter"] for r in steps] == list(range(1, 13)) and summary["done"] and summary["last_checkpoint"] == 12
        assert all(np.isfinite(r["loss"]) for r in steps), [r["loss"] for r in steps]
        assert steps[0]["lr"] == 5e-5 / 10 and steps[-1]["lr"] == 5e-5 / 10 * 9 * 0.5 * 0.5   # warm-up, then the milestones at 10 and 11
        for it in (6, 12):
            g_path = os.path.join(out, "models", "%d_G.pth" % it)
            assert os.path.exists(g_path) and os.path.exists(os.path.join(out, "training_state", "%d.state" % it))
            checkpoint.load_network(g_path, M.VQLLFLOWDeformable(), strict=True)
        val = steps[-1]["val"]
        assert val["images"] == 3 and np.isfinite(val["psnr"]) and np.isfinite(val["ssim"])
        rel = abs(steps[0]["loss"] - hand_a) / abs(hand_a)
        print("%s: step-1 loss %.9g, %.3g relative from the hand-fed step" % ("--graph" if graph else "eager", steps[0]["loss"], rel))
        assert rel <= bound, (steps[0]["loss"], hand_a, rel, bound)
    st = torch.load(os.path.join(out, "training_state", "6.state"), map_location="cpu", weights_only=False)
    assert st["iter"] == 6 and st["epoch"] == 1 and st["optimizers"][0]["param_groups"][0]["betas"] == (0.9, 0.99)


def test_stage2_through_the_driver_and_resume(tmp_path):
    """11. niter 4 at 2 x 320^2: finite losses, a checkpoint, and a resume that runs 2 more steps."""
    root = str(tmp_path / "data")
    make_v1(root, "our485", [(330, 340), (320, 320), (350, 325)], seed=3)
    out = str(tmp_path / "run")
    recs = _run("stage2", root, out, tmp_path, "--niter", "4", "--batch", "2", "--save-freq", "4")
    assert [r["iter"] for r in recs[:-1]] == [1, 2, 3, 4] and all(np.isfinite(r["loss"]) for r in recs[:-1]), recs
    state = os.path.join(out, "training_state", "4.state")
    assert os.path.exists(state) and os.path.exists(os.path.join(out, "models", "4_G.pth"))
    recs = _run("stage2", root, out, tmp_path, "--niter", "6", "--batch", "2", "--save-freq", "4", "--resume", state)
    assert [r["iter"] for r in recs[:-1]] == [5, 6] and all(np.isfinite(r["loss"]) for r in recs[:-1]), recs
    assert os.path.exists(os.path.join(out, "training_state", "6.state"))
