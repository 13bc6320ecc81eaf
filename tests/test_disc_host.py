"""Host side of the stage-1 GAN term: no GPU.  The new ops have no CPU path, the driver's switches are refused where they do not apply,
a plain stage-1 run builds no discriminator, and every new export is declared in the header the binding is derived from."""
import pytest
import torch

from glare_amd import _lib, fit
from glare_amd import autograd as A
from glare_amd import train_ops as T

NEW_EXPORTS = ("glare_conv4x4_packed_elems", "glare_conv4x4_pack_bf16", "glare_conv4x4_forward_bf16", "glare_conv4x4_dgrad_bf16",
               "glare_conv4x4_im2col_t_bf16", "glare_batchnorm_workspace_bytes", "glare_batchnorm_lrelu_bf16",
               "glare_batchnorm_lrelu_backward_bf16", "glare_lrelu_backward_bf16", "glare_hinge_workspace_bytes", "glare_hinge_loss_f32")


def test_new_ops_have_no_cpu_path():
    x16, x32 = torch.zeros(1, 6, 6, 8, dtype=torch.bfloat16), torch.zeros(1, 6, 6, 3)
    w8, w3 = torch.zeros(8, 8, 4, 4), torch.zeros(8, 3, 4, 4)
    g, b = torch.ones(8), torch.zeros(8)
    calls = [lambda: T.conv4x4_pack(w8), lambda: T.conv4x4_forward(x16, w8), lambda: T.conv4x4_forward(x32, w3, b, stride=1, lrelu=True),
             lambda: T.conv4x4_dgrad(x16[:, :3, :3].contiguous(), w8, (1, 6, 6, 8)), lambda: T.conv4x4_im2col_t(x16, 2),
             lambda: T.conv4x4_weight_grad(x16, x16[:, :3, :3].contiguous(), 8, 2), lambda: T.lrelu_backward(x16, x16),
             lambda: T.batchnorm_forward(x16, g, b), lambda: T.batchnorm_backward(x16, x16, torch.zeros(1, 2, 8), g, b),
             lambda: T.hinge_loss(torch.zeros(5), "real"), lambda: A.conv4x4(x32, w3, None), lambda: A.batchnorm_lrelu(x16, g, b),
             lambda: A.hinge_loss(torch.zeros(5), "generator")]
    for i, call in enumerate(calls):
        with pytest.raises(NotImplementedError):
            call()
            pytest.fail("call %d ran on CPU tensors" % i)


def test_discriminator_module_is_tamings_and_has_no_cpu_path():
    from disc_oracle import sequential
    from glare_amd.modules import NLayerDiscriminator

    torch.manual_seed(0)
    d, ref = NLayerDiscriminator(), sequential()
    assert list(d.state_dict()) == ["main." + k for k in ref.state_dict()]
    assert {k: tuple(v.shape) for k, v in d.main.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    ref.load_state_dict(d.main.state_dict(), strict=True)
    w = d.main[8].weight.detach()
    assert abs(float(w.std()) - 0.02) < 1e-3 and abs(float(w.mean())) < 1e-3                  # N(0, 0.02)
    assert abs(float(d.main[9].weight.mean()) - 1.0) < 5e-3 and float(d.main[9].bias.abs().max()) == 0.0
    with pytest.raises(NotImplementedError):
        d.train_nhwc(torch.zeros(1, 64, 64, 3))
    assert tuple(ref(torch.zeros(1, 3, 256, 256)).shape) == (1, 1, 30, 30) and tuple(ref(torch.zeros(1, 3, 64, 64)).shape) == (1, 1, 6, 6)


@pytest.mark.parametrize("stage", ("stage2", "stage3"))
def test_gan_is_refused_outside_stage1(stage, capsys):
    with pytest.raises(SystemExit):
        fit.parse_args([stage, "--root", "r", "--out", "o", "--gan"])
    assert "--gan is a stage1 option" in capsys.readouterr().err
    with pytest.raises(ValueError, match="stage1 option"):
        fit.build_trainer(stage, fit.default_options(stage), torch.device("cpu"), gan=True)


def test_gan_switches():
    args, options = fit.parse_args(["stage1", "--root", "r", "--out", "o", "--gan", "--disc-start", "7", "--disc-weight", "0.5"])
    assert args.gan and options["train"]["disc_start"] == 7 and options["train"]["disc_weight"] == 0.5
    args, options = fit.parse_args(["stage1", "--root", "r", "--out", "o"])
    assert not args.gan and "disc_start" not in options["train"]
    with pytest.raises(SystemExit):
        fit.parse_args(["stage1", "--root", "r", "--out", "o", "--disc-start", "7"])           # needs --gan
    with pytest.raises(SystemExit):
        fit.parse_args(["stage1", "--root", "r", "--out", "o", "--gan", "--graph"])            # --graph stays refused


def test_plain_stage1_builds_no_discriminator():
    tr = fit.build_trainer("stage1", fit.default_options("stage1"), torch.device("cpu"))
    assert tr.discriminator is None and tr.opt_d is None and len(tr.opt.groups) == 2
    assert not any("discriminator" in n or n.startswith("main.") for n, _ in tr.netG.named_parameters())


def test_header_declares_every_new_export():
    sigs = _lib.signatures()
    for name in NEW_EXPORTS:
        assert name in sigs, name
    assert sigs["glare_hinge_loss_f32"][1][1] is _lib._SCALARS["long long"] and len(sigs["glare_conv4x4_forward_bf16"][1]) == 16
