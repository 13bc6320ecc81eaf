"""GPU: the patch discriminator as a network and the GAN step of Stage1Trainer against their CPU restatements in plain torch
(tests/disc_oracle.py for D, oracle.torch_ref's VQModel for the generator), and the driver's `--gan` checkpoints.
Every test here failed on the parent commit: the module, the trainer's keywords and the driver's switch did not exist.

Bounds: relative L2 per tensor, the metric of tests/test_gpu_stage1.py; each bound is twice the largest value measured on the MI355X over
three seeds (the project's rule), the measured values next to it and in DESIGN.md section 9."""
import json
import os

import numpy as np
import pytest
import torch

import disc_oracle as R
from test_gpu_stage1 import LOSS_SCALE, _dev, _rel
from tolerances import within

pytestmark = pytest.mark.gpu

SEEDS = (11, 12, 13)
# {precision: {quantity: bound}}, bound = 2 x the largest of the values measured over SEEDS and both shapes (in the comments)
NET_TOL = {"fp16": {"logits": 6.1e-3, "dx": 7.6e-2, "param_median": 6.5e-2, "param_max": 9.2e-2},      # measured 3.00e-3 / 3.77e-2 / 3.24e-2 / 4.60e-2
           "bf16": {"logits": 3.1e-2, "dx": 0.23, "param_median": 0.2, "param_max": 0.29}}             # measured 1.51e-2 / 0.114 / 0.0961 / 0.144
# Both precisions exceed what test_gpu_stage1.py allows the generator's parameters (fp16 4.6e-3 / 2.8e-2, bf16 3.4e-2 / 0.2).  It is the
# 16-bit format, not a kernel: the oracle Sequential with nothing changed but its activations, activation gradients and filters rounded to
# the 16-bit format where this path stores them gives, on the CPU in torch, fp16 2.9e-3 / 3.8e-2 / 3.2e-2 / 4.7e-2 and bf16 1.5e-2 / 0.113 /
# 0.095 / 0.146 for the same four figures, seeds and shapes.  Three BatchNorm backward passes (dz - mean dz - xhat mean
# dz xhat cancels most of dz) over small batches, behind LeakyReLU kinks, amplify a rounding that GroupNorm + swish pass on unamplified;
# every kernel by itself sits inside 0.5 ulp + its fp32 slack (test_gpu_disc_kernels.py).
STEP_TOL = {"fp16": {"g_loss": 1.6e-2, "d_loss": 8.5e-4, "d_weight": 1.3e-2, "gen_median": 0.21, "gen_max": 0.42, "disc_max": 0.17},
            # measured 7.60e-3 / 4.25e-4 / 6.31e-3 / 0.102 / 0.208 / 0.0836
            "bf16": {"g_loss": 2.8e-2, "d_loss": 4.9e-3, "d_weight": 0.112, "gen_median": 0.58, "gen_max": 1.04, "disc_max": 0.51}}
            # measured 1.38e-2 / 2.41e-3 / 5.56e-2 / 0.285 / 0.520 / 0.254.  The generator's total gradient is nll's plus d_weight x the gradient
            # that came back through D: D's d / dx carries the format error above (4 % / 11 %) on an input (xrec) that itself differs from the
            # oracle's by the generator's forward error, and LeakyReLU / BatchNorm make that gradient a non-smooth function of its input

def _pair(seed):
    """(HIP discriminator on the GPU, the oracle on the CPU) with the same taming initialisation."""
    from glare_amd import modules as M

    torch.manual_seed(seed)
    hip, ref = M.NLayerDiscriminator().train(), R.Discriminator().train()
    ref.load_state_dict(hip.state_dict(), strict=True)
    return hip.to(_dev()), ref


def _net_errors(prec, seed, shape):
    from glare_amd import ops

    hip, ref = _pair(seed)
    g = torch.Generator().manual_seed(seed)
    B, H, W = shape
    x = torch.rand(B, H, W, 3, generator=g)
    xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    out_r = ref(xr)
    w = torch.randn(out_r.shape, generator=g)
    (out_r * w).mean().backward()
    xd = x.to(_dev()).requires_grad_(True)
    with ops.use_precision(prec):
        out = hip.train_nhwc(xd)
        assert out.dtype == torch.float32 and tuple(out.shape) == (B, out_r.shape[2], out_r.shape[3], 1)
        ((out * w.permute(0, 2, 3, 1).to(_dev())).mean() * LOSS_SCALE[prec]).backward()
    errs = {}
    refp = dict(ref.named_parameters())
    for name, p in hip.named_parameters():
        assert p.grad is not None and refp[name].grad is not None, name
        errs[name] = _rel(p.grad / LOSS_SCALE[prec], refp[name].grad)
    vals = sorted(errs.values())
    res = {"logits": _rel(out.permute(0, 3, 1, 2), out_r), "dx": _rel(xd.grad.permute(0, 3, 1, 2) / LOSS_SCALE[prec], xr.grad),
           "param_median": vals[len(vals) // 2], "param_max": vals[-1]}
    # the running statistics moved as nn.BatchNorm2d's did
    for k, v in ref.state_dict().items():
        if "running" in k:
            assert _rel(hip.state_dict()[k], v) < 1e-2, k
        if "num_batches" in k:
            assert int(hip.state_dict()[k]) == int(v) == 1
    print("[%s seed %d %s]" % (prec, seed, "x".join(map(str, shape))), {k: "%.3e" % v for k, v in res.items()},
          "worst:", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    return res


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_network_gradients_match_the_oracle(prec):
    """Logits, d / dx and every parameter gradient of NLayerDiscriminator at 2 x 3 x 64^2 (6 x 6 logits) and 1 x 3 x 32 x 48 against fp32
    autograd of the oracle Sequential, loss = mean(logits * fixed weights)."""
    worst = {}
    for shape in ((2, 64, 64), (1, 32, 48)):
        for seed in SEEDS:
            for k, v in _net_errors(prec, seed, shape).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("[%s] largest over seeds and shapes:" % prec, {k: "%.3e" % v for k, v in worst.items()})
    for k, v in worst.items():
        within(v, NET_TOL[prec][k], "%s:%s" % (prec, k))


def test_logit_map_sizes():
    hip, _ = _pair(1)
    with torch.no_grad():
        assert tuple(hip.train_nhwc(torch.rand(1, 256, 256, 3, device=_dev())).shape) == (1, 30, 30, 1)
        assert tuple(hip(torch.rand(1, 3, 64, 64, device=_dev())).shape) == (1, 1, 6, 6)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def _trainer(precision, seed=6, disc_seed=3, **kw):
    from glare_amd import modules as M
    from glare_amd.synthetic import seeded_init_
    from glare_amd.train import Stage1Trainer

    if kw.pop("gan", True):
        torch.manual_seed(disc_seed)
        kw["discriminator"] = M.NLayerDiscriminator().to(_dev())
    tr = Stage1Trainer(seeded_init_(M.VQModel().train(), seed).to(_dev()), precision=precision, **kw)
    if precision == "fp16":                  # as tests/test_gpu_stage1.py: a scale no step of this toy problem overflows at
        tr.opt.scale.fill_(1024.0)
        if tr.opt_d is not None:
            tr.opt_d.scale.fill_(1024.0)
    return tr


def _batch(seed=31, B=2, S=64):
    return torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(seed)).to(_dev())


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_before_disc_start_the_step_is_the_plain_one(precision):
    x = _batch()
    tr, plain = _trainer(precision, disc_start=10), _trainer(precision, gan=False)
    d0 = {k: v.clone() for k, v in tr.discriminator.state_dict().items()}
    for _ in range(3):
        a, b = tr.step_tensor(x), plain.step_tensor(x)
        assert torch.equal(a, b)
    assert torch.equal(tr.opt.groups[0].w, plain.opt.groups[0].w) and torch.equal(tr.opt.groups[0].m, plain.opt.groups[0].m)
    assert torch.equal(tr.opt.groups[0].v, plain.opt.groups[0].v) and tr.opt.t == plain.opt.t == 3
    for k, v in tr.discriminator.state_dict().items():                       # parameters and running statistics untouched
        assert torch.equal(v, d0[k]), k
    g = tr.opt_d.groups[0]
    assert tr.opt_d.t == 0 and float(g.m.abs().max()) == 0.0 and float(g.v.abs().max()) == 0.0 and float(g.g.abs().max()) == 0.0
    assert set(tr.last_terms) == {"l1_loss", "codebook_loss", "g_loss", "d_weight", "d_loss"} and set(plain.last_terms) == {"l1_loss", "codebook_loss"}
    assert all(torch.is_tensor(tr.last_terms[k]) and tr.last_terms[k].is_cuda and float(tr.last_terms[k]) == 0.0 for k in ("g_loss", "d_weight", "d_loss"))
    assert tr.global_step == 3


def _step_errors(prec, seed):
    """One GAN step (disc_start = 0) against the whole step restated in torch on the CPU: trainer docstring / the issue's section 3."""
    from glare_amd import modules as M
    from glare_amd import ops
    from glare_amd.synthetic import seeded_init_
    from glare_amd.train import Stage1Trainer
    from oracle import torch_ref as O

    g = torch.Generator().manual_seed(seed)
    hip, ref = seeded_init_(M.VQModel().train(), 6), seeded_init_(O.VQModel().train(), 6)
    x = torch.rand(2, 3, 64, 64, generator=g)
    with torch.no_grad():
        sigma = float(ref.encode(x)[0].std())
    E = torch.randn(8192, 3, generator=g) * sigma                   # as test_autoencoder_gradients_match_the_oracle: tokens spread over the codes
    hip.quantize.embedding.weight.data.copy_(E)
    ref.quantize.embedding.weight.data.copy_(E)
    hipD, refD = _pair(seed)
    disc_weight, f, cw = 0.8, 1.0, 1.0
    tr = Stage1Trainer(hip.to(_dev()), precision=prec, discriminator=hipD, disc_start=0, disc_weight=disc_weight, disc_factor=f, codebook_weight=cw)
    scale = 1.0
    if prec == "fp16":
        scale = 1024.0
        tr.opt.scale.fill_(scale)
        tr.opt_d.scale.fill_(scale)
    xd = x.to(_dev())
    with ops.use_precision(prec):
        idx = tr.net.train_nhwc(xd)[2].cpu()                        # the HIP forward's indices: the oracle is built on them (no token left out)
    tr.step_tensor(xd)
    assert not tr.opt.last_step_skipped() and not tr.opt_d.last_step_skipped() and tr.opt.t == 1 and tr.opt_d.t == 1

    beta = ref.quantize.beta
    zp = ref.quant_conv(ref.encoder(x)).permute(0, 2, 3, 1).contiguous()
    zq = ref.quantize.embedding(idx).view(zp.shape)
    rq = beta * torch.mean((zq.detach() - zp) ** 2) + torch.mean((zq - zp.detach()) ** 2)
    zst = zp + (zq - zp).detach()
    dec, _ = ref.decoder(ref.post_quant_conv(zst.permute(0, 3, 1, 2).contiguous()))
    nll = (dec - x).abs().mean()
    g_loss = -refD(dec).mean()
    w_last = ref.decoder.conv_out.weight
    n_nll = torch.autograd.grad(nll, w_last, retain_graph=True)[0].norm()
    n_gan = torch.autograd.grad(g_loss, w_last, retain_graph=True)[0].norm()
    d_weight = (n_nll / (n_gan + 1e-4)).clamp(0.0, 1e4).detach() * disc_weight
    loss = nll + d_weight * f * g_loss + cw * rq
    gen = [(n, p) for n, p in ref.named_parameters() if not n.startswith("conv_semantic.")]
    ggen = torch.autograd.grad(loss, [p for _, p in gen], allow_unused=True)
    d_loss = f * 0.5 * (torch.relu(1.0 - refD(x)).mean() + torch.relu(1.0 + refD(dec.detach())).mean())
    gdisc = torch.autograd.grad(d_loss, list(refD.parameters()))

    hipp = dict(tr.net.named_parameters())
    gen_errs = {}
    for (name, _), gr in zip(gen, ggen):
        if gr is None or name.endswith(".k.bias"):                  # (softmax does not depend on k's bias: rounding noise on both sides)
            continue
        gen_errs[name] = _rel(hipp[name].grad / scale, gr)
    disc_errs = {n: _rel(p.grad / scale, gr) for (n, p), gr in zip(tr.discriminator.named_parameters(), gdisc)}
    vals = sorted(gen_errs.values())
    rel1 = lambda a, b: abs(float(a.detach()) - float(b.detach())) / abs(float(b.detach()))
    res = {"g_loss": rel1(tr.last_terms["g_loss"], g_loss), "d_loss": rel1(tr.last_terms["d_loss"], d_loss),
           "d_weight": rel1(tr.last_terms["d_weight"], d_weight), "gen_median": vals[len(vals) // 2], "gen_max": vals[-1],
           "disc_max": max(disc_errs.values())}
    print("[%s seed %d] g_loss %.6g (oracle %.6g) d_loss %.6g (%.6g) d_weight %.6g (%.6g)" % (
        prec, seed, float(tr.last_terms["g_loss"]), float(g_loss), float(tr.last_terms["d_loss"]), float(d_loss),
        float(tr.last_terms["d_weight"]), float(d_weight)), {k: "%.3e" % v for k, v in res.items()},
        "worst gen:", sorted(gen_errs.items(), key=lambda kv: -kv[1])[:3], "worst disc:", sorted(disc_errs.items(), key=lambda kv: -kv[1])[:3])
    return res


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_gan_step_matches_the_oracle(prec):
    worst = {}
    for seed in SEEDS:
        for k, v in _step_errors(prec, seed).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("[%s] largest over seeds:" % prec, {k: "%.3e" % v for k, v in worst.items()})
    for k, v in worst.items():
        within(v, STEP_TOL[prec][k], "%s:%s" % (prec, k))


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_discriminator_learns_a_fixed_batch(precision):
    """The generator frozen (its reconstruction computed once, its parameters never touched): 20 updates of D on one batch."""
    from glare_amd import ops

    tr = _trainer(precision, lr_G=1e-3, disc_start=0)
    x = _batch(41)
    with ops.use_precision(precision), torch.no_grad():
        xrec = tr.net.train_nhwc(x)[0].detach().clone()
    w0 = tr.opt.groups[0].w.clone()
    losses = [float(tr.discriminator_step(x, xrec)) for _ in range(20)]
    print(precision, ["%.4f" % l for l in losses])
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
    assert all(bool(torch.isfinite(l).all()) for l in tr.last_logits)
    assert torch.equal(tr.opt.groups[0].w, w0) and tr.opt_d.t == 20 and tr.opt.t == 0
    assert int(tr.discriminator.main[3].num_batches_tracked) == 40           # two batch groups per pass


def _folders(tmp_path):
    from PIL import Image

    rng = np.random.default_rng(4)
    root = str(tmp_path / "data")
    for split, sizes in (("our485", [(70, 90), (64, 64), (81, 66)]), ("eval15", [(44, 76)])):
        for sub in ("low", "high"):
            os.makedirs(os.path.join(root, split, sub))
            for i, (h, w) in enumerate(sizes):
                Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(root, split, sub, "%02d.png" % i))
    opt = str(tmp_path / "opt.json")
    with open(opt, "w") as f:
        json.dump({"logger": {"print_freq": 1}, "datasets": {"train": {"GT_size": 64}}}, f)
    return root, opt


def test_driver_gan_checkpoints_and_bitwise_resume(tmp_path):
    """`fit stage1 --gan --disc-start 1` at 2 x 64^2: four steps in one run against two steps, save, resume, two more -- the same bits in
    the generator and in D; `<iter>_D.pth` is taming's state dict; the JSON lines carry the three terms."""
    from glare_amd import fit

    root, opt = _folders(tmp_path)
    base = ["stage1", "--root", root, "--opt", opt, "--batch", "2", "--save-freq", "2", "--no-val", "--gan", "--disc-start", "1"]
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    recs = fit.main(base + ["--out", one, "--niter", "4"])
    steps = recs[:-1]
    assert [r["iter"] for r in steps] == [1, 2, 3, 4] and all(np.isfinite(r["loss"]) for r in steps), steps
    assert all({"g_loss", "d_weight", "d_loss"} <= set(r) for r in steps)
    assert steps[0]["d_loss"] == 0.0 and steps[0]["d_weight"] == 0.0 and steps[1]["d_loss"] > 0.0 and steps[1]["d_weight"] > 0.0
    assert sorted(os.listdir(os.path.join(one, "models"))) == ["2_D.pth", "2_VQ.pth", "4_D.pth", "4_VQ.pth"]
    sd = torch.load(os.path.join(one, "models", "4_D.pth"), map_location="cpu")
    ref = R.Discriminator()
    assert list(sd) == list(ref.state_dict()) and all(not v.is_cuda for v in sd.values())
    ref.load_state_dict(sd, strict=True)
    st = torch.load(os.path.join(one, "training_state", "2.state"), map_location="cpu", weights_only=False)
    assert st["discriminator"]["optimizer"]["param_groups"][0]["betas"] == (0.5, 0.9) and "scale" in st["discriminator"]["scaler"]
    assert len(st["discriminator"]["optimizer"]["state"]) == len(list(ref.parameters()))

    fit.main(base + ["--out", two, "--niter", "2"])
    recs2 = fit.main(base + ["--out", two, "--niter", "4", "--resume", os.path.join(two, "training_state", "2.state")])
    assert [r["iter"] for r in recs2[:-1]] == [3, 4]
    for name in ("4_VQ.pth", "4_D.pth"):
        a = torch.load(os.path.join(one, "models", name), map_location="cpu")
        b = torch.load(os.path.join(two, "models", name), map_location="cpu")
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)
    assert [r["loss"] for r in recs2[:-1]] == [r["loss"] for r in steps[2:]]
