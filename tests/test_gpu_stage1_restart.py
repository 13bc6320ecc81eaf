"""GPU: Stage1Trainer(codebook_restart=P) at 2 x 64^2 (N = 512 tokens, K = 8192 codes; the fixture style of tests/test_gpu_stage1.py) -- a
run that never restarts against a trainer without the option, a restart against tests/vq_restart_oracle.py applied to a twin trainer's
buffers, the GAN step, the histogram shared with codebook_usage, the resume mid-window and its refusals, and the driver end to end.
Every comparison is on bits."""
import json
import os

import numpy as np
import pytest
import torch

import vq_restart_oracle as R
from glare_amd import checkpoint, evaluate, fit, ops, train
from glare_amd import modules as M
from glare_amd.synthetic import seeded_init_
from glare_amd.train import Stage1Trainer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K, N = 8192, 512


def _trainer(**kw):
    tr = Stage1Trainer(seeded_init_(M.VQModel().train(), 6).to(DEV), precision="fp16", **kw)
    tr.opt.scale.fill_(1024.0)          # as tests/test_gpu_stage1.py: a scale no step of this toy problem overflows at
    if tr.opt_d is not None:
        tr.opt_d.scale.fill_(1024.0)
    return tr


def _batch(seed=31, B=2, S=64):
    return torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def _rows(tr):
    """The embedding's rows of the flat w, exp_avg and exp_avg_sq of group 0, found from the parameter itself."""
    E, g = tr.net.quantize.embedding.weight, tr.opt.groups[0]
    off = (E.data_ptr() - g.w.data_ptr()) // 4
    assert 0 <= off and off + E.numel() <= g.w.numel()
    return tuple(t[off:off + E.numel()].view(K, 3) for t in (g.w, g.m, g.v))


def _same_state(a, b):
    ga, gb = a.opt.groups[0], b.opt.groups[0]
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in ((ga.w, gb.w), (ga.m, gb.m), (ga.v, gb.v)))


def _hist(tr):
    return np.bincount(tr.net.last_indices.cpu().numpy(), minlength=K).astype(np.int64)


def test_a_run_that_never_restarts_is_the_run_without_the_option():
    plain, never = _trainer(), _trainer(codebook_restart=10 ** 9)
    assert plain.log_terms() == () and never.log_terms() == ("codebook_restarted",) and plain.restart_window is None
    x = _batch()
    for _ in range(2):
        a, b = plain.step_tensor(x), never.step_tensor(x)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert set(plain.last_terms) == {"l1_loss", "codebook_loss"} and int(never.last_terms["codebook_restarted"]) == 0
    assert _same_state(plain, never)
    assert int(never.restart_window.sum()) == 2 * N and plain.extra_state() == {}


def _run_and_check_restarts(make, x):
    """4 steps at P = 2 of make(codebook_restart=2) beside make(codebook_restart=10**9): the first restart against the restatement applied to
    the twin's buffers (the twin IS the trainer up to the restart), the second by its own rows."""
    tr, twin = make(codebook_restart=2), make(codebook_restart=10 ** 9)
    window = np.zeros(K, np.int64)
    for step in (1, 2, 3, 4):
        tr.step_tensor(x)
        n = tr.last_terms["codebook_restarted"]
        assert n.is_cuda and n.dtype == torch.int64 and n.dim() == 0
        window += _hist(tr)
        z = tr.net.last_latent
        assert z.dtype == torch.float32 and tuple(z.shape) == (N, 3) and not z.requires_grad
        if step <= 2:
            twin.step_tensor(x)
        if step % 2:
            assert int(n) == 0 and np.array_equal(tr.restart_window.cpu().numpy(), window), step
            if step == 1:
                assert _same_state(tr, twin)
            continue
        w, m, v = _rows(tr)
        z_np = z.cpu().numpy()
        offset = (step // 2) * 7919
        if step == 2:
            assert np.array_equal(twin.restart_window.cpu().numpy(), window)             # snapshotted before the call: the twin's
            tw, tm, tv = (t.cpu().numpy() for t in _rows(twin))
            want = R.restart(window, 0, z_np, offset, tw, tm, tv)
            assert np.array_equal(_bits(w), want["codebook"].view(np.uint32))
            assert np.array_equal(_bits(m), want["exp_avg"].view(np.uint32)) and np.array_equal(_bits(v), want["exp_avg_sq"].view(np.uint32))
            # ... and nothing else of the flat buffers moved
            gt, gw = tr.opt.groups[0], twin.opt.groups[0]
            off = (w.data_ptr() - gt.w.data_ptr()) // 4
            for a, b in ((gt.w, gw.w), (gt.m, gw.m), (gt.v, gw.v)):
                assert torch.equal(a[:off], b[:off]) and torch.equal(a[off + 3 * K:], b[off + 3 * K:])
        else:
            want = R.restart(window, 0, z_np, offset, w.cpu().numpy())
        print("step", step, "dead", want["n_dead"], "restarted", want["n_restarted"])
        assert int(n) == want["n_restarted"] > 0 and want["n_dead"] > 0
        rows, tokens = want["rows"], want["tokens"]
        assert np.array_equal(_bits(w)[rows], z_np.view(np.uint32)[tokens])              # the re-seeded rows are those latent rows
        assert not _bits(m)[rows].any() and not _bits(v)[rows].any()                     # +0.0
        assert not bool(tr.restart_window.any())
        window[:] = 0
    return tr


def test_a_restart_run_matches_the_restatement():
    tr = _run_and_check_restarts(_trainer, _batch())
    assert tr.global_step == 4 and tr.opt.t == 4
    assert set(tr.last_terms) == {"l1_loss", "codebook_loss", "codebook_restarted"}


def test_the_gan_step_restarts_too():
    def make(**kw):
        torch.manual_seed(3)
        return _trainer(discriminator=M.NLayerDiscriminator().to(DEV), disc_start=0, **kw)

    tr = _run_and_check_restarts(make, _batch(33))
    assert set(tr.last_terms) == {"l1_loss", "codebook_loss", "g_loss", "d_weight", "d_loss", "codebook_restarted"}
    assert tr.log_terms() == ("g_loss", "d_weight", "d_loss", "codebook_restarted")


def test_restart_and_usage_share_one_histogram_call(monkeypatch):
    calls = []
    real = ops.vq_usage

    def counted(*a, **kw):
        calls.append(kw.get("total"))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "vq_usage", counted)
    x = _batch()
    usage, both, alone = _trainer(codebook_usage=True), _trainer(codebook_usage=True, codebook_restart=2), _trainer(codebook_restart=2)
    for tr, total in ((usage, None), (both, both.restart_window), (alone, alone.restart_window)):
        for step in (1, 2):
            del calls[:]
            tr.step_tensor(x)
            assert len(calls) == 1 and calls[0] is total, (step, len(calls))             # one histogram launch pair per step
    usage, both = _trainer(codebook_usage=True), _trainer(codebook_usage=True, codebook_restart=2)
    usage.step_tensor(x)
    both.step_tensor(x)
    assert int(both.last_terms["codebook_active"]) == int(usage.last_terms["codebook_active"]) == int((_hist(both) > 0).sum())
    assert float(both.last_terms["codebook_perplexity"]) == float(usage.last_terms["codebook_perplexity"])
    assert np.array_equal(both.restart_window.cpu().numpy(), _hist(both))
    assert both.log_terms() == ("codebook_active", "codebook_perplexity", "codebook_restarted")


def test_resume_mid_window_continues_bit_for_bit(tmp_path):
    x = _batch(35)
    straight = _trainer(codebook_restart=2)
    for _ in range(4):
        straight.step_tensor(x)
    first = _trainer(codebook_restart=2)
    for _ in range(3):
        first.step_tensor(x)
    assert int(first.restart_window.sum()) == N                                          # mid-window: step 3's counts wait for step 4
    path = str(tmp_path / "3.state")
    checkpoint.save_training_state(path, first, 0, 3, extra=first.extra_state())
    st = torch.load(path, map_location="cpu", weights_only=False)
    saved = st[train.RESTART_KEY]
    assert saved["every"] == 2 and saved["threshold"] == 0 and saved["window"].dtype == torch.int64 and tuple(saved["window"].shape) == (K,)

    def resumed(**kw):
        tr = _trainer(**kw)
        tr.net.load_state_dict(first.net.state_dict())
        _, step = checkpoint.resume_training(st, tr)
        tr.on_resume(step)
        tr.load_extra_state(st)
        return tr

    second = resumed(codebook_restart=2)
    assert torch.equal(second.restart_window, first.restart_window) and second.global_step == 3
    second.step_tensor(x)
    assert int(second.last_terms["codebook_restarted"]) == int(straight.last_terms["codebook_restarted"]) > 0
    assert _same_state(straight, second) and torch.equal(straight.restart_window, second.restart_window)
    for a, b in zip(_rows(straight), _rows(second)):
        assert np.array_equal(_bits(a), _bits(b))
    # the refusals
    with pytest.raises(AssertionError, match="codebook-restart"):
        resumed(codebook_restart=3)                                                      # another `every`
    with pytest.raises(AssertionError, match="codebook-restart"):
        resumed(codebook_restart=2, restart_threshold=1)                                 # another threshold
    with pytest.raises(AssertionError, match="codebook-restart"):
        resumed()                                                                        # the key without the option
    del st[train.RESTART_KEY]
    with pytest.raises(AssertionError, match="codebook-restart"):
        resumed(codebook_restart=2)                                                      # the option without the key
    resumed()                                                                            # neither: as ever


def test_driver_with_codebook_restart_end_to_end(tmp_path):
    """`python -m glare_amd.fit stage1 ... --codebook-restart 2 --batch 2`, 4 steps at 2 x 64^2 on synthetic folders: every JSON line carries
    `codebook_restarted`, the checkpoint is a plain VQModel's, and glare_amd.evaluate stage1 scores the run as any other."""
    from PIL import Image

    rng = np.random.default_rng(4)
    root, out = str(tmp_path / "data"), str(tmp_path / "run")
    for split, sizes in (("our485", [(70, 90), (64, 64), (81, 66)]), ("eval15", [(44, 76), (44, 76)])):     # (evaluate stacks the split)
        for sub in ("low", "high"):
            os.makedirs(os.path.join(root, split, sub))
            for i, (h, w) in enumerate(sizes):
                Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(root, split, sub, "%02d.png" % i))
    opt = str(tmp_path / "opt.json")
    with open(opt, "w") as f:
        json.dump({"logger": {"print_freq": 1}, "datasets": {"train": {"GT_size": 64}}}, f)
    recs = fit.main(["stage1", "--root", root, "--out", out, "--opt", opt, "--batch", "2", "--save-freq", "4", "--niter", "4",
                     "--codebook-restart", "2", "--no-val"])
    steps = recs[:-1]
    assert [r["iter"] for r in steps] == [1, 2, 3, 4] and all("codebook_restarted" in r for r in steps)
    assert json.loads(json.dumps(recs)) == recs
    got = [r["codebook_restarted"] for r in steps]
    print("codebook_restarted per step:", got)
    assert got[0] == got[2] == 0 and got[1] > 0 and got[3] > 0 and all(np.isfinite(r["loss"]) for r in steps)
    assert sorted(os.listdir(os.path.join(out, "models"))) == ["4_VQ.pth"]
    checkpoint.load_network(os.path.join(out, "models", "4_VQ.pth"), M.VQModel(), strict=True)
    st = torch.load(os.path.join(out, "training_state", "4.state"), map_location="cpu", weights_only=False)
    assert st[train.RESTART_KEY]["every"] == 2 and int(st[train.RESTART_KEY]["window"].sum()) == 0       # step 4 restarted
    res = evaluate.main(["stage1", "--run", out, "--root", root, "--batch", "1"])
    assert res["stage"] == "stage1" and res["images"] == 2 and [c["name"] for c in res["checkpoints"]] == ["4_VQ"]
    assert np.isfinite(res["checkpoints"][0]["means"]["PSNR"]) and set(res["checkpoints"][0]["codebook"]) == set(evaluate.USAGE_KEYS)
    # a resume without the option, and the option for another stage, are refused
    with pytest.raises(AssertionError, match="codebook-restart"):
        fit.main(["stage1", "--root", root, "--out", out, "--opt", opt, "--batch", "2", "--niter", "5", "--no-val",
                  "--resume", os.path.join(out, "training_state", "4.state")])
