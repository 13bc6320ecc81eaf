"""GPU: the LPIPS term as a network (losses.LPIPSLoss against tests/lpips_oracle.py on the CPU), inside a Stage1Trainer step (against
oracle.torch_ref's VQModel + the LPIPS oracle, with and without the discriminator) and through the driver (`fit stage1 --vgg16 F
--lpips-heads G`, `fit stage3 --vgg16 F`).  Every test here failed on the parent commit: losses.LPIPSLoss did not exist.

Scope: the published weights cannot be obtained offline.  The arithmetic is pinned to a restatement of the published definition on
name-seeded weights; agreement with the pretrained model's absolute values is not pinned and not claimed.

Bounds: relative L2, the metric of tests/test_gpu_stage1.py.
  network   value and d / dxrec: exactly twice what the oracle's 16-bit rounding emulation shows for that quantity and precision on the
            CPU (lpips_oracle.EMULATED_ERR, held to the computation within 2 % by tests/test_lpips_host.py), three seeds x three shapes.
  step      l1_loss: within LOSS_TOL x (l1 + codebook) absolutely -- test_gpu_stage1's LOSS_TOL is the relative bound of that sum on
            the plain step, l1 is all but 7e-4 of it, and the autoencoder's forward is untouched.
            codebook_loss: relative to itself, CODEBOOK_TOL.  The term is (1 + beta) mean (zq - zp)^2 on the HIP step's own indices:
            its error is the 16-bit encoder's error in zp, which no test bounds on its own, so the bound is the project's rule for such
            a pin -- twice the figure measured on the MI355X, of code this term does not change.
            percep_loss, twice: against the oracle evaluated on the HIP step's own reconstruction, the network's value bound; against
            the CPU step, that bound plus what the autoencoder's forward error can move the oracle's LPIPS by,
            2 |d lpips / d xrec| |xrec_hip - xrec_cpu| / lpips (Cauchy-Schwarz on the oracle's own gradient; the 2 covers the gradient's
            change between the two reconstructions, which the emulation puts at 16 % for a far larger perturbation).
            Parameter gradients, per tensor: test_gpu_stage1's largest-tensor bound for the plain step PLUS the two errors the term
            adds to THAT tensor, both computed here on the CPU from the oracle alone -- twice the first, an emulation, and once the
            second, which is exact (the triangle inequality through the oracle at the HIP step's reconstruction):
              rounding -- the oracle's step (fp32 autoencoder) with the emulated LPIPS against the same with the fp32 LPIPS
                          (lpips_oracle.term_rounding_errors; its median and largest at the oracle's own indices are pinned on the
                          host as lpips_oracle.EMULATED_STEP_ERR);
              moved    -- the oracle's step with d lpips / d xrec taken at the HIP step's reconstruction against the same taken at the
                          oracle's own.  The term is evaluated where the 16-bit autoencoder put xrec, 5e-4 (fp16) / 4e-3 (bf16) from
                          the oracle's, which is the size of one 16-bit rounding: behind 13 ReLUs and 4 max-pools the gradient of
                          LPIPS moves under it as it does under the rounding (decisions flip), while its value hardly does.
            No bound is above GRAD_CAP = 0.9: a gradient that is all zero scores 1.0 and an unrelated one of the right size 1.4, so
            no tensor's bound lets either pass (under bf16 the rounding alone is 58 % at quant_conv / post_quant_conv, whose bound is
            therefore the cap).  Their median: the plain step's median bound plus the two medians, weighed alike.  The issue words the
            gradient bounds as the plain step's scaled by a ratio of d / dxrec errors with and without the term; the plain step's
            seed, sign(xrec - x) / n, is exact in fp32, so that ratio has no denominator and the sources of error are added instead.
  GAN step  d_weight against the CPU step within test_gpu_disc's d_weight bound; it must differ from the L1-only run's.
Measured on the MI355X: next to each bound and in DESIGN.md section 9."""
import json
import os

import numpy as np
import pytest
import torch

import lpips_oracle as R
from test_gpu_disc import STEP_TOL, _folders, _pair
from test_gpu_stage1 import GRAD_TOL, LOSS_SCALE, LOSS_TOL, _dev, _rel
from tolerances import within

pytestmark = pytest.mark.gpu

DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}
NET_TOL = {p: {k: 2 * R.EMULATED_ERR[p][k] for k in ("value", "dx")} for p in ("fp16", "bf16")}
CODEBOOK_TOL = {"fp16": 2.65e-3, "bf16": 1.97e-2}     # codebook_loss relative to itself: twice the measured 1.325e-3 / 9.856e-3
GRAD_CAP = 0.9                                        # a zero gradient scores 1.0
# measured on the MI355X (largest over seeds and shapes): fp16 value 1.90e-4 / dx 5.34e-2 (bounds 3.96e-4 / 0.108), bf16 2.15e-3 / 0.154 (5.12e-3 / 0.312).
# The step at seed 11, fp16 | bf16: l1 4.9e-7 | 4.9e-4 of l1 + codebook (bound 5.5e-5 | 1.1e-3); percep at the HIP reconstruction 2.1e-5 | 3.0e-5,
# against the CPU step 2.1e-5 | 5.6e-4 (bound 5.4e-3 | 4.5e-2); gradients: median 5.3e-2 | 0.147 (bound 0.111 | 0.315; the rounding's median
# 2.6e-2 | 7.2e-2, the moved reconstruction's 5.4e-2 | 0.137), largest measured / bound over the 248 tensors 0.54 | 0.60, largest error 0.129 | 0.537
# (quant_conv / post_quant_conv; 2 bf16 bounds are the cap).  d_weight 0.3968 | 0.4012 against 0.4085 | 0.4133 for the L1-only nll; against the CPU
# step 6.0e-3 (bound 1.3e-2) | 2.1e-2 (bound 0.112).


def _hip_lpips(sd):
    from glare_amd import losses

    net = losses.LPIPSLoss()
    back, heads = R.torchvision_form(sd)
    assert len(losses.load_vgg16(net, back, heads)) == 31
    return net.to(_dev())


def _oracle(sd):
    ref = R.LPIPS()
    ref.load_state_dict(sd, strict=True)
    return ref


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_network_matches_the_oracle(prec):
    from glare_amd import ops

    worst = {"value": 0.0, "dx": 0.0}
    for seed in R.NET_SEEDS:
        sd = R.seeded_state(seed)
        hip, ref = _hip_lpips(sd), _oracle(sd)
        for shape in R.NET_SHAPES:
            xrec, x = R.net_case(seed, shape)
            xr = xrec.clone().requires_grad_(True)
            v_ref = ref(xr, x)
            (g_ref,) = torch.autograd.grad(v_ref, xr)
            xd = xrec.permute(0, 2, 3, 1).contiguous().to(_dev()).requires_grad_(True)
            with ops.use_precision(prec):
                v = hip(xd, x.permute(0, 2, 3, 1).contiguous().to(_dev()))
                assert v.dim() == 0 and v.dtype == torch.float32
                (v * LOSS_SCALE[prec]).backward()
            got = {"value": _rel(v, v_ref), "dx": _rel(xd.grad.permute(0, 3, 1, 2) / LOSS_SCALE[prec], g_ref)}
            print("[%s seed %d %s] lpips %.6g (oracle %.6g)" % (prec, seed, "x".join(map(str, shape)), float(v), float(v_ref)),
                  {k: "%.3e" % e for k, e in got.items()})
            assert bool(torch.isfinite(xd.grad).all())
            for k, e in got.items():
                worst[k] = max(worst[k], e)
    print("[%s] largest over seeds and shapes:" % prec, {k: "%.3e" % e for k, e in worst.items()}, "bounds", NET_TOL[prec])
    for k, e in worst.items():
        within(e, NET_TOL[prec][k], "%s:%s" % (prec, k))


def test_frozen_filters_are_packed_once_not_once_per_step(monkeypatch):
    """The launch list of the filter packs: the first forward + backward packs each of the trunk's 12 MFMA convs per direction (and the
    first conv's data gradient), the second and third pack nothing; a weight load packs again."""
    from glare_amd import losses, ops

    packs = []
    real = ops.PackedConv

    class Recording(real):
        __slots__ = ()

        def __init__(self, weight_oihw=None, bias=None, dgrad_pad=None, **kw):
            if weight_oihw is not None:
                packs.append((tuple(weight_oihw.shape), dgrad_pad))
            super().__init__(weight_oihw, bias, dgrad_pad=dgrad_pad, **kw)

    monkeypatch.setattr(ops, "PackedConv", Recording)
    sd = R.seeded_state(11)
    hip = _hip_lpips(sd)
    xrec, x = R.net_case(11, (1, 32, 48))
    xd, x0 = xrec.permute(0, 2, 3, 1).contiguous().to(_dev()), x.permute(0, 2, 3, 1).contiguous().to(_dev())
    values = []
    with ops.use_precision("fp16"):
        for step in range(3):
            n0 = len(packs)
            xs = xd.clone().requires_grad_(True)
            v = hip(xs, x0)
            (v * 1024.0).backward()
            values.append((float(v), xs.grad.clone()))
            print("step %d: %d filter packs" % (step, len(packs) - n0))
            if step == 0:
                first = packs[n0:]
                assert len([p for p in first if p[1] is None]) == 12                                                # forward: conv 2 .. 13
                assert len([p for p in first if p[1] is not None]) == 13                                            # data gradient: all 13
            else:
                assert len(packs) == n0
        assert values[0][0] == values[1][0] == values[2][0] and torch.equal(values[0][1], values[2][1])
        # new weights in place (what load_vgg16 does): seen, packed again, and the value moves
        back, heads = R.torchvision_form(R.seeded_state(12))
        losses.load_vgg16(hip, back, heads)
        n0 = len(packs)
        v = hip(xd.clone().requires_grad_(True), x0)
        assert len(packs) - n0 == 12 and float(v) != values[0][0]
        # a filter whose storage is replaced (p.data = ...) is packed again from the new storage, not served the old pack
        conv = getattr(hip.net.slice2, "5")
        conv.weight.data = conv.weight.data * 2.0
        n0 = len(packs)
        v2 = hip(xd.clone().requires_grad_(True), x0)
        assert len(packs) - n0 == 1 and float(v2) != float(v)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def _step_errors(prec, seed, gan):
    """One Stage1Trainer(perceptual=LPIPSLoss) step at 1 x 3 x 64 x 64 against the step restated in torch on the CPU."""
    from glare_amd import modules as M
    from glare_amd import ops
    from glare_amd.synthetic import seeded_init_
    from glare_amd.train import Stage1Trainer
    from oracle import torch_ref as O

    g = torch.Generator().manual_seed(seed)
    hip, ref = seeded_init_(M.VQModel().train(), 6), seeded_init_(O.VQModel().train(), 6)
    x = torch.rand(1, 3, 64, 64, generator=g)
    with torch.no_grad():
        sigma = float(ref.encode(x)[0].std())
    E = torch.randn(8192, 3, generator=g) * sigma                   # as test_autoencoder_gradients_match_the_oracle: tokens spread over the codes
    hip.quantize.embedding.weight.data.copy_(E)
    ref.quantize.embedding.weight.data.copy_(E)
    sd = R.seeded_state(seed)
    lp_hip, lp_ref = _hip_lpips(sd), _oracle(sd)
    pw, cw, disc_weight, f = 1.0, 1.0, 0.8, 1.0
    kw = {}
    if gan:
        hipD, refD = _pair(seed)
        kw = dict(discriminator=hipD, disc_start=0, disc_weight=disc_weight, disc_factor=f)
    hip = hip.to(_dev())

    def trainer(perceptual):
        tr = Stage1Trainer(hip, precision=prec, perceptual=perceptual, perceptual_weight=pw, codebook_weight=cw, **kw)
        if prec == "fp16":
            tr.opt.scale.fill_(1024.0)
            if tr.opt_d is not None:
                tr.opt_d.scale.fill_(1024.0)
        return tr

    xd = x.to(_dev())
    res = {}
    if gan:
        # the L1-only run's adaptive weight, on the same networks (a step moves them: snapshot and put back)
        snap = {k: v.clone() for k, v in hip.state_dict().items()}
        snapD = {k: v.clone() for k, v in hipD.state_dict().items()}
        tr0 = trainer(None)
        tr0.step_tensor(xd)
        res["d_weight_l1_only"] = float(tr0.last_terms["d_weight"])
        hip.load_state_dict(snap)
        hipD.load_state_dict(snapD)
        hip.invalidate()
        hipD.invalidate()
    tr = trainer(lp_hip)
    scale = 1024.0 if prec == "fp16" else 1.0
    with ops.use_precision(prec):
        xrec_hip, _, idx = tr.net.train_nhwc(xd)                    # the HIP forward's reconstruction and indices (the oracle is built on them)
        xrec_hip, idx = xrec_hip.detach().permute(0, 3, 1, 2).float().cpu(), idx.cpu()
    tr.step_tensor(xd)
    assert not tr.opt.last_step_skipped() and tr.opt.t == 1

    beta = ref.quantize.beta
    zp = ref.quant_conv(ref.encoder(x)).permute(0, 2, 3, 1).contiguous()
    zq = ref.quantize.embedding(idx).view(zp.shape)
    rq = beta * torch.mean((zq.detach() - zp) ** 2) + torch.mean((zq - zp.detach()) ** 2)
    zst = zp + (zq - zp).detach()
    dec, _ = ref.decoder(ref.post_quant_conv(zst.permute(0, 3, 1, 2).contiguous()))
    l1 = (dec - x).abs().mean()
    percep = pw * lp_ref(dec, x)
    nll = l1 + percep
    loss = nll + cw * rq
    if gan:
        g_loss = -refD(dec).mean()
        w_last = ref.decoder.conv_out.weight
        n_nll = torch.autograd.grad(nll, w_last, retain_graph=True)[0].norm()
        n_gan = torch.autograd.grad(g_loss, w_last, retain_graph=True)[0].norm()
        d_weight = (n_nll / (n_gan + 1e-4)).clamp(0.0, 1e4).detach() * disc_weight
        loss = loss + d_weight * f * g_loss
    gen = [(n, p) for n, p in ref.named_parameters() if not n.startswith("conv_semantic.")]
    ggen = torch.autograd.grad(loss, [p for _, p in gen], allow_unused=True, retain_graph=True)
    with torch.no_grad():
        percep_at_hip = pw * lp_ref(xrec_hip, x)
    (g_percep,) = torch.autograd.grad(percep, dec, retain_graph=True)
    forward_moves_percep = 2 * float(g_percep.norm() * (xrec_hip - dec.detach()).norm() / percep.detach().abs())
    emu, moved = {}, {}
    if not gan:      # the two sources of gradient error the term adds, each from the oracle alone (pw = 1)
        emu = R.term_rounding_errors(DTYPE[prec], gen, l1 + cw * rq, dec, x, lp_ref)
        xh = xrec_hip.clone().requires_grad_(True)
        (g_at_hip,) = torch.autograd.grad(pw * lp_ref(xh, x), xh)
        gmoved = torch.autograd.grad([l1 + cw * rq, dec], [p for _, p in gen], [torch.ones(()), g_at_hip], allow_unused=True, retain_graph=True)
        moved = {n: _rel(a, b) for (n, _), a, b in zip(gen, gmoved, ggen) if b is not None}

    hipp = dict(tr.net.named_parameters())
    errs = {}
    for (name, _), gr in zip(gen, ggen):
        if gr is None or name.endswith(".k.bias"):
            continue
        errs[name] = _rel(hipp[name].grad / scale, gr)
    vals = sorted(errs.values())
    rel1 = lambda a, b: abs(float(a.detach()) - float(b.detach())) / abs(float(b.detach()))
    terms = tr.last_terms
    assert set(terms) >= {"l1_loss", "percep_loss", "codebook_loss"}
    res.update(l1_loss=rel1(terms["l1_loss"], l1), codebook_loss=rel1(terms["codebook_loss"], cw * rq),
               percep_loss=rel1(terms["percep_loss"], percep_at_hip), percep_vs_cpu_step=rel1(terms["percep_loss"], percep),
               forward_moves_percep=forward_moves_percep, median=vals[len(vals) // 2], max=vals[-1], sum=float(l1.detach() + cw * rq.detach()),
               l1_abs=abs(float(terms["l1_loss"]) - float(l1.detach())), codebook_abs=abs(float(terms["codebook_loss"]) - float(cw * rq.detach())))
    if gan:
        res["d_weight"] = rel1(terms["d_weight"], d_weight)
        res["d_weight_value"] = float(terms["d_weight"])
    print("[%s seed %d gan %d] l1 %.6g (oracle %.6g) percep %.6g (%.6g; at the HIP xrec %.6g) codebook %.6g (%.6g)" % (
        prec, seed, gan, float(terms["l1_loss"]), float(l1), float(terms["percep_loss"]), float(percep), float(percep_at_hip),
        float(terms["codebook_loss"]), float(cw * rq)), {k: "%.3e" % v for k, v in res.items()},
        "worst:", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    if not gan:
        assert set(emu) == set(errs)
        res["per_tensor"] = {n: (errs[n], min(GRAD_TOL[prec][1] + 2 * emu[n] + moved[n], GRAD_CAP)) for n in errs}
        med = lambda d: sorted(d[n] for n in errs)[len(errs) // 2]
        res["median_bound"] = GRAD_TOL[prec][0] + 2 * med(emu) + med(moved)
        print("[%s] per tensor, measured / bound (largest): %.3f;" % (prec, max(e / b for e, b in res["per_tensor"].values())),
              {n: "%.3g / %.3g (rounding %.3g, moved %.3g)" % (e, b, emu[n], moved[n])
               for n, (e, b) in sorted(res["per_tensor"].items(), key=lambda kv: -kv[1][0] / kv[1][1])[:8]},
              "medians: rounding %.4g, moved %.4g, bound %.4g; bounds at the cap: %d of %d" % (
                  med(emu), med(moved), res["median_bound"], sum(b == GRAD_CAP for _, b in res["per_tensor"].values()), len(errs)))
    return res


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_trainer_step_matches_the_cpu_step(prec):
    res = _step_errors(prec, 11, gan=False)
    within(res["l1_abs"] / res["sum"], LOSS_TOL[prec], prec + ":l1")
    within(res["codebook_loss"], CODEBOOK_TOL[prec], prec + ":codebook")
    within(res["percep_loss"], NET_TOL[prec]["value"], prec + ":percep")
    within(res["percep_vs_cpu_step"], NET_TOL[prec]["value"] + res["forward_moves_percep"], prec + ":percep_vs_cpu_step")
    assert NET_TOL[prec]["value"] + res["forward_moves_percep"] < 0.5                              # ... which is a bound worth the name
    within(res["median"], res["median_bound"], prec + ":median")
    for name, (err, bound) in res["per_tensor"].items():
        within(err, bound, "%s:%s" % (prec, name))


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_gan_step_weighs_the_discriminator_against_the_nll_with_the_term(prec):
    res = _step_errors(prec, 11, gan=True)
    assert res["d_weight_value"] != res["d_weight_l1_only"] and res["d_weight_value"] > 0       # nll now contains the term
    print("[%s] d_weight with LPIPS %.6g, L1 only %.6g" % (prec, res["d_weight_value"], res["d_weight_l1_only"]))
    within(res["d_weight"], STEP_TOL[prec]["d_weight"], prec + ":d_weight")
    within(res["percep_loss"], NET_TOL[prec]["value"], prec + ":percep")
    within(res["percep_vs_cpu_step"], NET_TOL[prec]["value"] + res["forward_moves_percep"], prec + ":percep_vs_cpu_step")


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
def _weight_files(tmp_path, seed=11):
    sd = R.seeded_state(seed)
    back, heads = R.torchvision_form(sd)                            # torchvision / taming key form
    f, h = str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth")
    torch.save(back, f)
    torch.save(heads, h)
    return f, h, back


@pytest.mark.parametrize("gan", [False, True])
def test_driver_stage1_with_lpips_and_bitwise_resume(tmp_path, gan):
    from glare_amd import fit

    root, opt = _folders(tmp_path)
    f, h, _ = _weight_files(tmp_path)
    base = ["stage1", "--root", root, "--opt", opt, "--batch", "2", "--save-freq", "1", "--no-val", "--vgg16", f, "--lpips-heads", h]
    if gan:
        base += ["--gan", "--disc-start", "1"]
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    recs = fit.main(base + ["--out", one, "--niter", "3"])
    steps = recs[:-1]
    assert [r["iter"] for r in steps] == [1, 2, 3]
    assert all(np.isfinite(r["loss"]) and np.isfinite(r["percep_loss"]) and r["percep_loss"] > 0 for r in steps), steps
    names = ["%d_%s.pth" % (i, t) for i in (1, 2, 3) for t in (("D", "VQ") if gan else ("VQ",))]
    assert sorted(os.listdir(os.path.join(one, "models"))) == sorted(names)            # the loss network is written nowhere
    st = torch.load(os.path.join(one, "training_state", "2.state"), map_location="cpu", weights_only=False)
    assert not any("lin" in str(k) or "slice" in str(k) for k in st)
    fit.main(base + ["--out", two, "--niter", "2"])
    recs2 = fit.main(base + ["--out", two, "--niter", "3", "--resume", os.path.join(two, "training_state", "2.state")])   # names the files again
    assert [r["iter"] for r in recs2[:-1]] == [3] and recs2[0]["percep_loss"] == steps[2]["percep_loss"] and recs2[0]["loss"] == steps[2]["loss"]
    for name in names[-(2 if gan else 1):]:
        with open(os.path.join(one, "models", name), "rb") as fa, open(os.path.join(two, "models", name), "rb") as fb:
            assert fa.read() == fb.read(), name                                        # step 3's checkpoint bytes
    if not gan:      # the .state records that the run had the term: resumed without the files it is refused, not continued on L1 alone
        plain = [a for a in base if a not in ("--vgg16", f, "--lpips-heads", h)]
        with pytest.raises(ValueError, match="objective would change"):
            fit.main(plain + ["--out", two, "--niter", "3", "--resume", os.path.join(two, "training_state", "2.state")])


@pytest.mark.parametrize("graph", [False, True])
def test_driver_stage3_with_vgg16(tmp_path, monkeypatch, graph):
    from glare_amd import fit, losses

    root, opt = _folders(tmp_path)
    f, _, back = _weight_files(tmp_path)
    made = []
    real = fit.build_trainer
    monkeypatch.setattr(fit, "build_trainer", lambda *a, **k: made.append(real(*a, **k)) or made[-1])
    argv = ["stage3", "--root", root, "--out", str(tmp_path / "run"), "--opt", opt, "--batch", "2", "--niter", "2", "--no-val", "--vgg16", f]
    recs = fit.main(argv + (["--graph"] if graph else []))
    steps = recs[:-1]
    assert [r["iter"] for r in steps] == [1, 2] and all(np.isfinite(r["percep_loss"]) and r["percep_loss"] > 0 for r in steps), steps
    pn = made[0].perceptual
    assert isinstance(pn, losses.PerceptualNetwork) and not any(p.requires_grad for p in pn.parameters())
    sd = pn.state_dict()
    assert len(sd) == 14
    for k, v in sd.items():
        assert torch.equal(v.cpu(), back["features." + k.split(".", 1)[1]]), k
    assert sorted(os.listdir(str(tmp_path / "run" / "models"))) == ["2_G.pth"]
    with pytest.raises(SystemExit):
        fit.main(argv + ["--lpips-heads", f])
