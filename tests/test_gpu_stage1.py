"""GPU: stage 1, the VQGAN prior with a tape -- VectorQuantizer2.forward under grad, the gradient of the whole autoencoder against
fp32 autograd of the CPU oracle (oracle.torch_ref), and Stage1Trainer's mechanics."""
import numpy as np
import pytest
import torch

from tolerances import within

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LOSS_SCALE = {"bf16": 1.0, "fp16": 4096.0}       # as tests/test_gpu_train.py: what FlatAdam.scale_loss does for fp16 activation gradients


def _dev():
    return torch.device("cuda", 0)


def _gamma(n):
    return n * U / (1.0 - n * U)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _param_grad_errors(hip_mod, ref_mod, scale=1.0):
    """{parameter name: relative L2 error of its gradient}; a parameter the reference graph never reaches has no gradient here either."""
    errs = {}
    ref = dict(ref_mod.named_parameters())
    hip = dict(hip_mod.named_parameters())
    assert set(ref) == set(hip)
    for name, p in hip.items():
        if ref[name].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, name
        if name.endswith(".k.bias"):
            # softmax_j(q_i.(k_j + b)) does not depend on b: the true gradient is 0 and both sides hold rounding noise
            assert float(p.grad.norm()) < 1e-2 * float(hip[name[:-4] + "weight"].grad.norm()), name
            continue
        errs[name] = _rel(p.grad / scale, ref[name].grad)
    return errs


@pytest.mark.parametrize("legacy", [False, True])
def test_vector_quantizer_forward_under_grad_matches_the_oracle(legacy):
    """Values and both gradients of VectorQuantizer2.forward at 2 x 3 x 16 x 16 against O.VectorQuantizer2 on the same fp32 input (CPU
    autograd), codebook N(0, 1).  The oracle is fp32 too: each bound is the kernel's (tests/test_gpu_vq_train.py) plus the same again
    for the oracle's own roundings of the same sums.  Failed with NotImplementedError before the codebook layer had a tape."""
    from glare_amd import modules as M
    from oracle import torch_ref as O

    g = torch.Generator().manual_seed(3)
    K, beta = 8192, 0.25
    hip, ref = M.VectorQuantizer2(K, 3, beta, legacy=legacy), O.VectorQuantizer2(K, 3, beta, legacy=legacy)
    E = torch.randn(K, 3, generator=g)
    hip.embedding.weight.data.copy_(E)
    ref.embedding.weight.data.copy_(E)
    hip.to(_dev())
    z = torch.randn(2, 3, 16, 16, generator=g)
    w = torch.randn(2, 3, 16, 16, generator=g)
    gl = 3.0
    zr = z.clone().requires_grad_(True)
    rq, rloss, (_, _, ridx) = ref(zr)
    ((rq * w).sum() + gl * rloss).backward()
    zd = z.to(_dev()).requires_grad_(True)
    q, loss, (_, _, idx) = hip(zd)
    ((q * w.to(_dev())).sum() + gl * loss).backward()

    assert torch.equal(idx.cpu(), ridx) and q.shape == z.shape and loss.dim() == 0
    assert torch.equal(q.detach().cpu(), rq.detach())                                       # z + (z_q - z): the same two fp32 roundings
    N = 2 * 16 * 16
    within(abs(float(loss.detach()) - float(rloss.detach())) / (2 * _gamma(3 * N + 6) * float(rloss.detach())), 1.0, "loss")
    w_z, w_e = (1.0, beta) if legacy else (beta, 1.0)
    flat = lambda t: t.detach().double().cpu().permute(0, 2, 3, 1).reshape(-1, 3)
    z64, zq64, g64 = flat(z), E.double()[ridx], flat(w)
    t = gl * (2 * w_z / (3 * N)) * (z64 - zq64)
    bound = 2 * 2.0 ** -21 * (g64.abs() + t.abs())
    within(float(((flat(zd.grad) - flat(zr.grad)).abs() / bound).max()), 1.0, "dz")
    within(float(((flat(zd.grad) - (g64 + t)).abs() / (0.5 * bound)).max()), 1.0, "dz vs fp64")      # the kernel's bound alone
    mag = torch.zeros(K, 3, dtype=torch.float64).index_add_(0, ridx, (zq64 - z64).abs())
    count = torch.bincount(ridx, minlength=K)
    used = count > 0
    dE, rdE = hip.embedding.weight.grad.double().cpu(), ref.embedding.weight.grad.double()
    assert bool((dE[~used] == 0).all()) and bool((rdE[~used] == 0).all())
    bound = 2 * _gamma(count[used].double() + 3)[:, None] * gl * (2 * w_e / (3 * N)) * mag[used] + 1e-45
    within(float(((dE[used] - rdE[used]).abs() / bound).max()), 1.0, "dE")
    # without a tape the module is what it was: same values, no graph
    with torch.no_grad():
        q0, loss0, (_, _, idx0) = hip(z.to(_dev()))
    assert torch.equal(q0, q.detach()) and torch.equal(idx0, idx) and not q0.requires_grad
    assert abs(float(loss0) - float(loss.detach())) <= 1e-5 * float(loss0)        # torch's own mean of the same squares


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_autoencoder_gradients_match_the_oracle(prec):
    """Every VQModel parameter gradient of loss = mean |xrec - x| + qloss at B = 2, 64 x 64 (latent 16 x 16) against fp32 autograd of the
    oracle's own modules on the CPU, built on the HIP forward's indices (E[idx_hip], straight-through form) so that no token is left
    out.  The codebook is redrawn N(0, sigma), sigma the oracle latent's std: the seeded 0.7 would put most tokens on a few codes."""
    from glare_amd import modules as M
    from glare_amd import autograd as A
    from glare_amd import ops
    from glare_amd.synthetic import seeded_init_
    from oracle import torch_ref as O

    g = torch.Generator().manual_seed(21)
    hip, ref = seeded_init_(M.VQModel().train(), 6), seeded_init_(O.VQModel().train(), 6)
    x = torch.rand(2, 3, 64, 64, generator=g)
    with torch.no_grad():
        sigma = float(ref.encode(x)[0].std())
    E = torch.randn(8192, 3, generator=g) * sigma
    hip.quantize.embedding.weight.data.copy_(E)
    ref.quantize.embedding.weight.data.copy_(E)
    hip.to(_dev())

    with ops.use_precision(prec):
        xrec, qloss, idx = hip.train_nhwc(x.to(_dev()))
        loss = A.l1_loss(xrec, x.to(_dev())) + qloss
        (loss * LOSS_SCALE[prec]).backward()
    idx = idx.cpu()

    beta = ref.quantize.beta
    zp = ref.quant_conv(ref.encoder(x)).permute(0, 2, 3, 1).contiguous()
    with torch.no_grad():
        own = ref.quantize(zp.permute(0, 3, 1, 2))[2][2]
    zq = ref.quantize.embedding(idx).view(zp.shape)
    rq = beta * torch.mean((zq.detach() - zp) ** 2) + torch.mean((zq - zp.detach()) ** 2)
    zst = zp + (zq - zp).detach()
    dec, _ = ref.decoder(ref.post_quant_conv(zst.permute(0, 3, 1, 2).contiguous()))
    rloss = (dec - x).abs().mean() + rq
    rloss.backward()

    print("[%s] share of the HIP forward's indices equal to the oracle's own argmin: %.4f" % (prec, float((own == idx).float().mean())))
    loss, rloss, qloss, rq = loss.detach(), rloss.detach(), qloss.detach(), rq.detach()
    print("[%s] loss %.6f (oracle %.6f), qloss %.6f (oracle %.6f)" % (prec, float(loss), float(rloss), float(qloss), float(rq)))
    errs = _param_grad_errors(hip, ref, LOSS_SCALE[prec])
    assert "quantize.embedding.weight" in errs and "quant_conv.weight" in errs and "post_quant_conv.bias" in errs
    assert not any(n.startswith("conv_semantic.") for n in errs)
    vals = sorted(errs.values())
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    print("[%s] median %.4f max %.4f" % (prec, vals[len(vals) // 2], vals[-1]), worst)
    print("[%s] codebook layer:" % prec, {n: round(errs[n], 5) for n in errs if "quant" in n})
    within(abs(float(loss) - float(rloss)) / abs(float(rloss)), LOSS_TOL[prec], prec + ":loss")
    med_tol, max_tol = GRAD_TOL[prec]
    within(vals[len(vals) // 2], med_tol, prec + ":median")
    within(vals[-1], max_tol, prec + ":max")


# bounds = at most 2x the values measured on the MI355X (the project's rule); measured values in the comments
LOSS_TOL = {"fp16": 5.5e-5, "bf16": 1.1e-3}                          # measured 2.77e-05 / 5.54e-04 (relative, loss 0.6151 / 0.6142 vs 0.6152 / 0.6145)
GRAD_TOL = {"fp16": (4.6e-3, 2.8e-2), "bf16": (3.4e-2, 0.2)}         # (median, max) measured fp16 0.0023 / 0.0141, bf16 0.0172 / 0.1018; the max is
#                                                                      the codebook's (a 3-channel gradient through the 16-bit decoder), then the
#                                                                      encoder's first block; share of indices equal to the oracle's own argmin: 0.9844 / 0.8828


def _trainer(precision, seed=6, **kw):
    from glare_amd import modules as M
    from glare_amd.synthetic import seeded_init_
    from glare_amd.train import Stage1Trainer

    tr = Stage1Trainer(seeded_init_(M.VQModel().train(), seed).to(_dev()), precision=precision, **kw)
    if precision == "fp16":
        tr.opt.scale.fill_(1024.0)      # a scale no step of this toy problem overflows at: every step is applied (from GradScaler's
    return tr                           # initial 65536 the first steps may be skipped and halve it)


def _batch(seed=31, B=2, S=64):
    return torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(seed)).to(_dev())


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_stage1_trainer_steps_reduce_the_loss(precision):
    from glare_amd import modules as M

    tr = _trainer(precision)
    assert tr.opt.loss_scaling == (precision == "fp16") and tr.opt.betas == (0.5, 0.9)
    x = _batch()
    with torch.no_grad():
        z_before = tr.net.encode_nhwc(x).clone()                     # builds the packed inference weights the steps must invalidate
    cb0 = tr.net.quantize.embedding.weight.detach().clone()
    sem0 = tr.net.conv_semantic[0].weight.detach().clone()
    losses = [tr.step(x) for _ in range(8)]
    print(precision, losses, {k: float(v.detach()) for k, v in tr.last_terms.items()}, tr.opt.scaler_state_dict(), "steps applied:", tr.opt.t)
    assert all(l == l for l in losses) and losses[-1] < losses[0]
    assert tr.opt.t == 8 and set(tr.last_terms) == {"l1_loss", "codebook_loss"}
    assert not torch.equal(cb0, tr.net.quantize.embedding.weight.detach())           # the codebook trains ...
    assert torch.equal(sem0, tr.net.conv_semantic[0].weight.detach())                # ... the never-used branch does not move
    p0 = next(tr.net.parameters())
    assert p0.data_ptr() == tr.opt.groups[0].w.data_ptr()                            # views of the flat buffers
    # after a step the inference entry points run on the new weights (net.invalidate())
    fresh = M.VQModel().eval()
    fresh.load_state_dict(tr.net.state_dict())
    fresh.to(_dev())
    tr.net.eval()
    with torch.no_grad():
        z_after, z_fresh = tr.net.encode_nhwc(x), fresh.encode_nhwc(x)
        i_after, img_after, _ = tr.net.decode_nhwc(z_after, want_image=True)
        i_fresh, img_fresh, _ = fresh.decode_nhwc(z_fresh, want_image=True)
    assert torch.equal(z_after, z_fresh) and not torch.equal(z_after, z_before)
    assert torch.equal(i_after, i_fresh) and torch.equal(img_after, img_fresh)


def test_step_with_nonfinite_gradients_is_skipped():
    """An input scaled past fp16's range overflows the activations: the step's gradients hold inf / NaN, nothing moves, the scale
    backs off; the next ordinary step is applied."""
    tr = _trainer("fp16")
    x = _batch()
    tr.step(x)
    w0, t0, scale0 = tr.opt.groups[0].w.clone(), tr.opt.t, float(tr.opt.scale.item())
    tr.step_tensor(x * 1e6)
    assert tr.opt.last_step_skipped() and tr.opt.t == t0 and torch.equal(tr.opt.groups[0].w, w0)
    assert float(tr.opt.scale.item()) == 0.5 * scale0
    loss = tr.step(x)
    assert loss == loss and not tr.opt.last_step_skipped() and tr.opt.t == t0 + 1 and not torch.equal(tr.opt.groups[0].w, w0)
    assert bool(torch.isfinite(tr.opt.groups[0].w).all())


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_two_trainers_built_alike_stay_bit_identical(precision):
    finals = []
    for _ in range(2):
        tr = _trainer(precision)
        x = _batch(33)
        losses = [tr.step(x) for _ in range(3)]
        finals.append((losses, tr.opt.groups[0].w.clone(), tr.opt.groups[0].m.clone()))
    assert finals[0][0] == finals[1][0]
    assert torch.equal(finals[0][1], finals[1][1]) and torch.equal(finals[0][2], finals[1][2])


def test_one_step_at_the_reference_crop():
    tr = _trainer("fp16")
    loss = tr.step(_batch(35, B=4, S=256))
    assert np.isfinite(loss) and not tr.opt.last_step_skipped() and tr.opt.t == 1


def test_module_forward_is_the_taped_autoencoder():
    """VQModel.forward(input) -> (dec NCHW, diff) (VQModel_arch.py:98-101): under grad the tape, under no_grad decode(encode(input))."""
    from glare_amd import modules as M
    from glare_amd import ops
    from glare_amd.synthetic import seeded_init_

    net = seeded_init_(M.VQModel().train(), 6).to(_dev())
    x = _batch(37)
    with ops.use_precision("fp16"):
        dec, diff = net(x)
        assert dec.shape == x.shape and dec.requires_grad and diff.dim() == 0
        ((dec - x).abs().mean() + diff).backward()
    assert net.quantize.embedding.weight.grad is not None and net.encoder.conv_in.weight.grad is not None
    assert net.conv_semantic[0].weight.grad is None
    with torch.no_grad(), ops.use_precision("fp16"):
        dec0, diff0 = net(x)
    assert dec0.shape == x.shape and not dec0.requires_grad and bool(torch.isfinite(dec0).all()) and float(diff0) > 0


def test_driver_end_to_end_and_resume(tmp_path):
    """`python -m glare_amd.fit stage1` on synthetic folders: 3 steps at 2 x 64^2, checkpoints under the VQModel key names, the closing
    validation (PSNR of decode(encode(gt)) over the test split, one image with sides that are no multiple of 4), then a resume."""
    import json
    import os

    from PIL import Image

    from glare_amd import checkpoint, fit
    from glare_amd import modules as M

    rng = np.random.default_rng(4)
    root, out = str(tmp_path / "data"), str(tmp_path / "run")
    for split, sizes in (("our485", [(70, 90), (64, 64), (81, 66)]), ("eval15", [(44, 76), (45, 78)])):
        for sub in ("low", "high"):
            os.makedirs(os.path.join(root, split, sub))
            for i, (h, w) in enumerate(sizes):
                Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(root, split, sub, "%02d.png" % i))
    opt = str(tmp_path / "opt.json")
    with open(opt, "w") as f:
        json.dump({"logger": {"print_freq": 1}, "datasets": {"train": {"GT_size": 64}}}, f)
    args = ["stage1", "--root", root, "--out", out, "--opt", opt, "--batch", "2", "--save-freq", "2"]
    recs = fit.main(args + ["--niter", "3"])
    steps, summary = recs[:-1], recs[-1]
    assert [r["iter"] for r in steps] == [1, 2, 3] and summary["done"] and summary["last_checkpoint"] == 3
    assert all(np.isfinite(r["loss"]) for r in steps), steps
    assert steps[0]["lr"] == 1e-4 / 10                                       # the warm-up override on the stage's lr_G
    val = steps[-1]["val"]
    assert val["images"] == 2 and np.isfinite(val["psnr"]) and 0 < val["psnr"] < 100
    assert sorted(os.listdir(os.path.join(out, "models"))) == ["2_VQ.pth", "3_VQ.pth"]
    checkpoint.load_network(os.path.join(out, "models", "3_VQ.pth"), M.VQModel(), strict=True)
    state = os.path.join(out, "training_state", "2.state")
    st = torch.load(state, map_location="cpu", weights_only=False)
    assert st["iter"] == 2 and st["optimizers"][0]["param_groups"][0]["betas"] == (0.5, 0.9)
    assert len(st["optimizers"][0]["state"]) == len(list(M.VQModel().parameters())) - 2          # no Adam state for conv_semantic
    recs = fit.main(args + ["--niter", "4", "--resume", state, "--no-val"])
    assert [r["iter"] for r in recs[:-1]] == [3, 4] and all(np.isfinite(r["loss"]) for r in recs[:-1]), recs
    assert os.path.exists(os.path.join(out, "models", "4_VQ.pth"))
