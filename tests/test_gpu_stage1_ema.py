"""GPU: Stage1Trainer(codebook_ema=d) at 2 x 64^2 (N = 512 tokens, K = 8192 codes; the fixture of tests/test_gpu_stage1_restart.py) -- the
option off against a trainer built without it, every step's codebook, cluster_size and embed_avg against ops.vq_ema_stats + ops.vq_ema_update
applied to copies taken before the step, Adam's hands off the codebook, the codebook term, the GAN step, the restart under EMA, the resume and
its refusals, the checkpoint's keys and the driver end to end.  Every comparison of state is on bits."""
import json
import os

import numpy as np
import pytest
import torch

from glare_amd import checkpoint, fit, ops, train
from glare_amd import modules as M
from glare_amd.synthetic import seeded_init_
from glare_amd.train import Stage1Trainer
from tolerances import within

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K, N = 8192, 512
DECAY, EPS = 0.99, 1e-5
U = 2.0 ** -24


def _trainer(**kw):
    tr = Stage1Trainer(seeded_init_(M.VQModel().train(), 6).to(DEV), precision="fp16", **kw)
    tr.opt.scale.fill_(1024.0)          # as tests/test_gpu_stage1.py: a scale no step of this toy problem overflows at
    if tr.opt_d is not None:
        tr.opt_d.scale.fill_(1024.0)
    return tr


def _batch(seed=31, B=2, S=64):
    return torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rows(tr):
    """The embedding's rows of the flat w, exp_avg and exp_avg_sq of group 0, found from the parameter itself."""
    E, g = tr.net.quantize.embedding.weight, tr.opt.groups[0]
    off = (E.data_ptr() - g.w.data_ptr()) // 4
    assert 0 <= off and off + E.numel() <= g.w.numel()
    return off, tuple(t[off:off + E.numel()].view(K, 3) for t in (g.w, g.m, g.v))


def _same_state(a, b):
    ga, gb = a.opt.groups[0], b.opt.groups[0]
    return (all(_same(x, y) for x, y in ((ga.w, gb.w), (ga.m, gb.m), (ga.v, gb.v)))
            and _same(a.cluster_size, b.cluster_size) and _same(a.embed_avg, b.embed_avg))


def _ema_state(tr):
    return tr.net.quantize.embedding.weight.detach().clone(), tr.cluster_size.clone(), tr.embed_avg.clone()


def _apply_update(tr, E, cs, ea):
    """ops.vq_ema_stats + ops.vq_ema_update of the step `tr` just took, in place on the copies."""
    stats = ops.vq_ema_stats(tr.net.last_indices, tr.net.last_latent, K)
    assert int(stats[:, 3].sum()) == N
    ops.vq_ema_update(stats, cs, ea, E, DECAY, EPS)


def test_the_option_off_is_the_trainer_without_it():
    plain, off = _trainer(), _trainer(codebook_ema=None)
    assert plain.codebook_ema is None and plain.cluster_size is None and plain.embed_avg is None
    assert plain.net.quantize.embedding.weight.requires_grad and not plain.net.quantize.ema_update
    x = _batch()
    for _ in range(2):
        a, b = plain.step_tensor(x), off.step_tensor(x)
        assert _same(a, b) and set(plain.last_terms) == {"l1_loss", "codebook_loss"}
    ga, gb = plain.opt.groups[0], off.opt.groups[0]
    assert all(_same(p, q) for p, q in ((ga.w, gb.w), (ga.m, gb.m), (ga.v, gb.v)))
    assert plain.extra_state() == {} and off.extra_state() == {} and plain.log_terms() == ()
    _, (w, m, v) = _rows(plain)
    assert bool(m.any()) and bool(v.any())                           # without EMA the codebook IS an Adam parameter


def test_every_step_is_the_ema_update_and_adam_leaves_the_codebook_alone():
    tr = _trainer(codebook_ema=DECAY)
    x = _batch()
    E = tr.net.quantize.embedding.weight
    for step in (1, 2, 3):
        E_old = E.detach().clone()
        E0, cs0, ea0 = _ema_state(tr)
        tr.step_tensor(x)
        idx, z = tr.net.last_indices, tr.net.last_latent
        _apply_update(tr, E0, cs0, ea0)
        assert _same(E, E0) and _same(tr.cluster_size, cs0) and _same(tr.embed_avg, ea0), step
        # codebook_loss = beta mean((z_q - z)^2) over the rows the lookup used (the old ones).  The loss kernel's bound
        # (tests/test_gpu_vq_train.py): gamma_n of the sum of the 3N terms, n = 3N + 3; three more roundings follow the sum here:
        # the scale beta / 3N as a float, its product with the sum, the product with codebook_weight
        terms = (E_old[idx].double() - z.double()) ** 2
        want = 0.25 * float(terms.mean())
        n = 3 * N + 3 + 3
        got = float(tr.last_terms["codebook_loss"].detach())
        print("step", step, "codebook_loss", got, "fp64", want)
        within(abs(got - want) / (n * U / (1 - n * U) * want), 1.0, "codebook_loss")
    _check_ema_invariants(tr)
    assert set(tr.last_terms) == {"l1_loss", "codebook_loss"} and tr.log_terms() == () and tr.opt.t == 3


def _check_ema_invariants(tr):
    E = tr.net.quantize.embedding.weight
    off, (w, m, v) = _rows(tr)
    assert w.data_ptr() == E.data_ptr() and not E.requires_grad and E.grad is None
    assert tr.net.quantize.ema_update and tr.net.quantize.loss_weights() == (0.25, 0.0)
    assert all(hi <= off or lo >= off + 3 * K for lo, hi in tr.opt.groups[0].active_ranges())          # outside what Adam updates
    assert not bool(m.any()) and not bool(v.any())                                                      # its moments stay zero
    g = tr.opt.groups[0]
    assert bool(g.m[:off].any()) and bool(g.m[off + 3 * K:].any())                                      # ... and the others' do not


def test_the_gan_step_updates_the_same_way():
    torch.manual_seed(3)
    tr = _trainer(codebook_ema=DECAY, discriminator=M.NLayerDiscriminator().to(DEV), disc_start=0)
    x = _batch(33)
    for step in (1, 2):
        E0, cs0, ea0 = _ema_state(tr)
        tr.step_tensor(x)
        _apply_update(tr, E0, cs0, ea0)
        assert _same(tr.net.quantize.embedding.weight, E0) and _same(tr.cluster_size, cs0) and _same(tr.embed_avg, ea0), step
    _check_ema_invariants(tr)
    assert set(tr.last_terms) == {"l1_loss", "codebook_loss", "g_loss", "d_weight", "d_loss"}


def test_the_restart_under_ema_follows_vq_restart_ema():
    tr = _trainer(codebook_ema=DECAY, codebook_restart=2)
    x = _batch()
    E = tr.net.quantize.embedding.weight
    window = torch.zeros(K, dtype=torch.int64, device=DEV)
    rows = None
    for step in (1, 2, 3):
        E0, cs0, ea0 = _ema_state(tr)
        tr.step_tensor(x)
        idx, z = tr.net.last_indices, tr.net.last_latent
        window += torch.bincount(idx, minlength=K)
        _apply_update(tr, E0, cs0, ea0)
        n = tr.last_terms["codebook_restarted"]
        if step == 2:                                                # the restart, after this step's EMA update
            dead = torch.nonzero(window == 0).flatten()
            before = E0.clone()
            n_dead, n_restarted = ops.vq_restart_ema(window, z, E0, ea0, cs0, (step // 2) * train.RESTART_OFFSET_STEP, 0, 1.0)
            assert int(n) == int(n_restarted) == min(int(n_dead), N) > 0 and int(n_dead) == dead.numel()
            rows = dead[:int(n_restarted)]
            assert bool((cs0[rows] == 1.0).all()) and _same(E0[rows], ea0[rows]) and not _same(E0[rows], before[rows])
            assert not bool(tr.restart_window.any())
            print("step 2: dead", int(n_dead), "re-seeded", int(n_restarted), "max |E| before", float(before.abs().max()),
                  "after", float(E0.abs().max()))
        else:
            assert int(n) == 0
        if step == 3:                                                # the lookup of the step after selects re-seeded rows
            hit = float(torch.isin(idx, rows).float().mean())
            print("step 3: fraction of tokens on re-seeded rows", hit)
            assert hit > 0
        assert _same(E, E0) and _same(tr.cluster_size, cs0) and _same(tr.embed_avg, ea0), step
    _check_ema_invariants(tr)
    assert set(tr.last_terms) == {"l1_loss", "codebook_loss", "codebook_restarted"}


def test_resume_continues_bit_for_bit_and_refuses_other_settings(tmp_path):
    x = _batch(35)
    kw = dict(codebook_ema=DECAY, codebook_restart=2)
    straight = _trainer(**kw)
    for _ in range(4):
        straight.step_tensor(x)
    first = _trainer(**kw)
    for _ in range(2):
        first.step_tensor(x)
    path = str(tmp_path / "2.state")
    checkpoint.save_training_state(path, first, 0, 2, extra=first.extra_state())
    st = torch.load(path, map_location="cpu", weights_only=False)
    saved = st[train.EMA_KEY]
    assert set(saved) == {"cluster_size", "embed_avg", "decay", "eps"} and saved["decay"] == DECAY and saved["eps"] == EPS
    assert saved["cluster_size"].dtype == saved["embed_avg"].dtype == torch.float32
    assert tuple(saved["cluster_size"].shape) == (K,) and tuple(saved["embed_avg"].shape) == (K, 3) and train.RESTART_KEY in st

    def resumed(**kw):
        tr = _trainer(**kw)
        tr.net.load_state_dict(first.net.state_dict())
        _, step = checkpoint.resume_training(st, tr)
        tr.on_resume(step)
        tr.load_extra_state(st)
        return tr

    second = resumed(**kw)
    assert _same_state(first, second) and second.global_step == 2
    for _ in range(2):
        second.step_tensor(x)
    assert _same_state(straight, second) and torch.equal(straight.restart_window, second.restart_window)
    assert _same(straight.net.quantize.embedding.weight, second.net.quantize.embedding.weight)
    assert int(second.last_terms["codebook_restarted"]) == int(straight.last_terms["codebook_restarted"])
    # the refusals
    with pytest.raises(AssertionError, match="codebook-ema"):
        resumed(codebook_restart=2)                                                      # the key without the option
    with pytest.raises(AssertionError, match="name the same values again"):
        resumed(codebook_ema=0.9, codebook_restart=2)                                    # another decay
    with pytest.raises(AssertionError, match="name the same values again"):
        resumed(codebook_ema=DECAY, ema_eps=1e-6, codebook_restart=2)                    # another eps
    del st[train.EMA_KEY]
    with pytest.raises(AssertionError, match="codebook-ema"):
        resumed(**kw)                                                                    # the option without the key
    resumed(codebook_restart=2)                                                          # neither: as ever


def test_driver_with_codebook_ema_end_to_end(tmp_path):
    """`python -m glare_amd.fit stage1 ... --codebook-ema 0.99 --codebook-restart 2 --batch 2`, 2 steps at 2 x 64^2 on synthetic folders:
    its JSON lines, a checkpoint with exactly VQModel's keys, and the EMA state in the `.state` file."""
    from PIL import Image

    rng = np.random.default_rng(4)
    root, out = str(tmp_path / "data"), str(tmp_path / "run")
    for split, sizes in (("our485", [(70, 90), (64, 64), (81, 66)]), ("eval15", [(44, 76)])):
        for sub in ("low", "high"):
            os.makedirs(os.path.join(root, split, sub))
            for i, (h, w) in enumerate(sizes):
                Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(root, split, sub, "%02d.png" % i))
    opt = str(tmp_path / "opt.json")
    with open(opt, "w") as f:
        json.dump({"logger": {"print_freq": 1}, "datasets": {"train": {"GT_size": 64}}}, f)
    argv = ["stage1", "--root", root, "--out", out, "--opt", opt, "--batch", "2", "--save-freq", "2", "--niter", "2", "--no-val"]
    recs = fit.main(argv + ["--codebook-ema", "0.99", "--codebook-restart", "2"])
    steps = recs[:-1]
    assert [r["iter"] for r in steps] == [1, 2] and json.loads(json.dumps(recs)) == recs
    assert all(np.isfinite(r["loss"]) for r in steps) and all(set(r) >= {"epoch", "iter", "lr", "loss", "ms_per_step", "codebook_restarted"} for r in steps)
    assert steps[0]["codebook_restarted"] == 0 and steps[1]["codebook_restarted"] > 0
    assert sorted(os.listdir(os.path.join(out, "models"))) == ["2_VQ.pth"]
    sd = torch.load(os.path.join(out, "models", "2_VQ.pth"), map_location="cpu", weights_only=False)
    assert set(sd) == set(M.VQModel().state_dict())                                      # what --net-vq and evaluate stage1 read
    checkpoint.load_network(os.path.join(out, "models", "2_VQ.pth"), M.VQModel(), strict=True)
    st = torch.load(os.path.join(out, "training_state", "2.state"), map_location="cpu", weights_only=False)
    ema = st[train.EMA_KEY]
    assert ema["decay"] == 0.99 and ema["eps"] == 1e-5 and float(ema["cluster_size"].sum()) > 0 and train.RESTART_KEY in st
    assert bool(torch.isfinite(sd["quantize.embedding.weight"]).all())
    # a resume without the option is refused
    with pytest.raises(AssertionError, match="codebook-ema"):
        fit.main(argv[:-3] + ["--niter", "3", "--no-val", "--codebook-restart", "2", "--resume", os.path.join(out, "training_state", "2.state")])
