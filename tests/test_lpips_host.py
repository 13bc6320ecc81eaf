"""Host: the LPIPS term's definitions and plumbing without a GPU -- the module layout against the oracle (tests/lpips_oracle.py), the fp64
reference of the head (tests/lpips_fp64.py) against fp64 autograd with and without an all-zero pixel, the strict loader, the driver's
refusals, and the rounding emulation that the network-level bounds of tests/test_gpu_lpips.py are taken from.
Every test imports a name the parent commit lacks (losses.LPIPSLoss, losses.load_vgg16, fit.check_perceptual_options, the two new
test modules)."""
import pytest
import torch

import lpips_fp64 as R64
import lpips_oracle as R
from glare_amd import fit, losses


def test_state_dict_has_the_published_keys_and_shapes():
    ours, ref = losses.LPIPSLoss().state_dict(), R.LPIPS().state_dict()
    assert list(ours) == list(ref)
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    assert torch.equal(ours["scaling_layer.shift"], ref["scaling_layer.shift"]) and torch.equal(ours["scaling_layer.scale"], ref["scaling_layer.scale"])
    net = losses.LPIPSLoss()
    assert not net.training and not net.train().training and not any(p.requires_grad for p in net.parameters())
    assert len([k for k in ours if k.startswith("net.")]) == 26 and [ours["lin%d.model.1.weight" % k].shape[1] for k in range(5)] == [64, 128, 256, 512, 512]


def _case(seed=5, shape=(2, 5, 7, 64)):
    g = torch.Generator().manual_seed(seed)
    a = torch.relu(torch.randn(shape, generator=g, dtype=torch.float64))
    b = torch.relu(torch.randn(shape, generator=g, dtype=torch.float64))
    w = torch.rand(shape[-1], generator=g, dtype=torch.float64)
    gi = torch.randn(shape[0], generator=g, dtype=torch.float64)
    return a, b, w, gi


def test_fp64_reference_equals_autograd_of_the_published_head():
    a, b, w, gi = _case()
    ref = R64.head64(a, b, w, gi)
    out, da = R64.head_autograd64(a, b, w, gi)
    assert float((ref["out"] - out).abs().max() / out.abs().max()) < 1e-12
    assert float((ref["da"] - da).abs().max() / da.abs().max()) < 1e-12
    # ... and the oracle's NCHW head is the same function
    out_nchw = R.head(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), w)
    assert float((out_nchw - out).abs().max() / out.abs().max()) < 1e-12


def test_fp64_reference_writes_zero_where_autograd_is_nan():
    a, b, w, gi = _case(6)
    a[1, 2, 3] = 0.0            # an all-zero pixel of the differentiated side
    b[0, 4, 1] = 0.0            # ... and of the constant side: nothing special
    ref = R64.head64(a, b, w, gi)
    out, da = R64.head_autograd64(a, b, w, gi)
    nan = torch.isnan(da)
    expect = torch.zeros_like(nan)
    expect[1, 2, 3] = True
    assert torch.equal(nan, expect)                                   # NaN exactly there, every channel of that pixel
    assert bool((ref["da"][1, 2, 3] == 0).all()) and bool(torch.isfinite(ref["da"]).all()) and bool(torch.isfinite(ref["out"]).all())
    assert float((ref["da"][~nan] - da[~nan]).abs().max() / da[~nan].abs().max()) < 1e-12
    assert float((ref["out"] - out).abs().max() / out.abs().max()) < 1e-12      # the forward value stays the finite one


def _forms(sd):
    back, heads = R.torchvision_form(sd)
    as_percep = {k.replace("features.", "vgg_model."): v for k, v in back.items()}
    as_lpips = {k: v for k, v in sd.items() if k.startswith("net.")}
    return back, as_percep, as_lpips, heads


def test_load_vgg16_takes_the_three_backbone_key_forms():
    sd = R.seeded_state(3)
    back, as_percep, as_lpips, heads = _forms(sd)
    back = dict(back, **{"classifier.0.weight": torch.zeros(4, 4)})            # what a torchvision file also holds: ignored
    for form in (back, as_percep, as_lpips):
        net = losses.LPIPSLoss()
        loaded = losses.load_vgg16(net, form, heads)
        assert sorted(loaded) == sorted(k for k in sd if not k.startswith("scaling_layer."))
        for k, v in net.state_dict().items():
            assert torch.equal(v, sd[k]), k
        pn = losses.PerceptualNetwork()
        loaded = losses.load_vgg16(pn, form)
        assert len(loaded) == 14
        for k, v in pn.state_dict().items():
            assert torch.equal(v, back["features." + k.split(".", 1)[1]]), k


def test_load_vgg16_from_files(tmp_path):
    sd = R.seeded_state(4)
    back, heads = R.torchvision_form(sd)
    f, h = str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth")
    torch.save(back, f)
    torch.save(heads, h)
    net = losses.LPIPSLoss()
    assert len(losses.load_vgg16(net, f, h)) == 31
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())


def test_load_vgg16_refuses_what_would_leave_a_tensor_at_its_initialisation():
    sd = R.seeded_state(3)
    back, _, _, heads = _forms(sd)
    lacking = {k: v for k, v in back.items() if not k.startswith("features.17.")}
    with pytest.raises(ValueError, match=r"features\.17\.weight"):
        losses.load_vgg16(losses.LPIPSLoss(), lacking, heads)
    with pytest.raises(ValueError, match="backbone"):                           # a heads file alone
        losses.load_vgg16(losses.LPIPSLoss(), None, heads)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight"):            # an LPIPSLoss without its heads
        losses.load_vgg16(losses.LPIPSLoss(), back)
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        losses.load_vgg16(losses.LPIPSLoss(), back, {k: v for k, v in heads.items() if not k.startswith("lin3.")})
    wrong = dict(back, **{"features.5.weight": torch.zeros(128, 64, 1, 1)})
    with pytest.raises(ValueError, match=r"features\.5\.weight.*\(128, 64, 1, 1\)"):
        losses.load_vgg16(losses.LPIPSLoss(), wrong, heads)
    with pytest.raises(ValueError, match="no LPIPS heads"):
        losses.load_vgg16(losses.PerceptualNetwork(), back, heads)
    with pytest.raises(ValueError, match=r"features\.14\."):                    # a PerceptualNetwork needs features[:16]
        losses.load_vgg16(losses.PerceptualNetwork(), {k: v for k, v in back.items() if not k.startswith("features.14.")})
    net = losses.LPIPSLoss()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    with pytest.raises(ValueError):
        losses.load_vgg16(net, lacking, heads)
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())  # a refused load copies nothing


@pytest.mark.parametrize("stage,kw,message", [
    ("stage1", dict(vgg16="a.pth"), fit.LPIPS_REFUSAL),
    ("stage1", dict(lpips_heads="b.pth"), fit.LPIPS_REFUSAL),
    ("stage3", dict(vgg16="a.pth", lpips_heads="b.pth"), fit.PERCEPTUAL_STAGE3_REFUSAL),
    ("stage3", dict(vgg16="a.pth", perceptual_weight=0.5), fit.PERCEPTUAL_STAGE3_REFUSAL),
    ("stage3", dict(lpips_heads="b.pth"), fit.PERCEPTUAL_STAGE3_REFUSAL),
    ("stage2", dict(vgg16="a.pth"), fit.PERCEPTUAL_STAGE2_REFUSAL),
    ("stage2", dict(lpips_heads="b.pth"), fit.PERCEPTUAL_STAGE2_REFUSAL),
    ("stage2", dict(perceptual_weight=1.0), fit.PERCEPTUAL_STAGE2_REFUSAL),
])
def test_driver_refusals(stage, kw, message):
    """build_trainer raises before it builds anything (no GPU, the files do not exist); the command line says the same."""
    with pytest.raises(ValueError) as e:
        fit.build_trainer(stage, fit.default_options(stage), torch.device("cpu"), **kw)
    assert str(e.value) == message
    argv = [stage, "--root", "r", "--out", "o"]
    for key, flag in (("vgg16", "--vgg16"), ("lpips_heads", "--lpips-heads"), ("perceptual_weight", "--perceptual-weight")):
        if key in kw:
            argv += [flag, str(kw[key])]
    with pytest.raises(SystemExit):
        fit.parse_args(argv)
    fit.check_perceptual_options(stage)                                          # none of the options: nothing to refuse
    fit.check_perceptual_options("stage1", "a.pth", "b.pth", 0.5)
    fit.check_perceptual_options("stage3", "a.pth")


@pytest.mark.parametrize("prec,dtype", [("fp16", torch.float16), ("bf16", torch.bfloat16)])
def test_rounding_emulation_is_the_source_of_the_network_bounds(prec, dtype):
    """The oracle with 16-bit rounding where the HIP path stores 16 bits, against the fp32 oracle, three seeds x three shapes: the table the
    GPU test doubles (lpips_oracle.EMULATED_ERR) is what this computes, rounded up in the third digit -- not below it, at most 2 % above."""
    got = R.emulation_errors(dtype)
    print(prec, {k: "%.3e" % v for k, v in got.items()}, "table", R.EMULATED_ERR[prec])
    for k, v in got.items():
        assert v <= R.EMULATED_ERR[prec][k] <= 1.02 * v, (prec, k, v, R.EMULATED_ERR[prec][k])


@pytest.mark.parametrize("prec,dtype", [("fp16", torch.float16), ("bf16", torch.bfloat16)])
def test_step_emulation_is_the_source_of_the_trainer_step_bounds(prec, dtype):
    """The oracle's stage-1 step (fp32 autoencoder) with the emulated LPIPS against the same step with the fp32 LPIPS: what the term's
    16-bit rounding alone does to the parameter gradients (median, largest).  tests/test_gpu_lpips.py adds the median, doubled, to the
    plain step's median bound and computes the per-tensor figures itself (lpips_oracle.term_rounding_errors) for the per-tensor bounds."""
    med, top = R.step_emulation_errors(dtype)
    print(prec, "median %.3e largest %.3e" % (med, top), "table", R.EMULATED_STEP_ERR[prec])
    for v, t in zip((med, top), R.EMULATED_STEP_ERR[prec]):
        assert v <= t <= 1.02 * v, (prec, v, t)
