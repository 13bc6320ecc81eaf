"""CPU: the host side of stage 1 (the VQGAN prior's training): the driver's command line and defaults, the loop's checkpoints under
the reference's VQModel key names and their resume with a stub step, the refusal of --graph, and the never-used parameter list
against what the CPU oracle's autograd actually reaches."""
import os
import types

import pytest
import torch

from glare_amd import checkpoint, fit, train
from glare_amd import modules as M
from glare_amd.train import STAGE1_NEVER_USED


def test_command_line_accepts_stage1(monkeypatch):
    args, options = fit.parse_args(["stage1", "--root", "data", "--out", "run", "--niter", "7", "--batch", "3", "--net-vq", "start.pth"])
    assert args.stage == "stage1" and args.net_vq == "start.pth" and not args.graph
    assert options["train"]["niter"] == 7 and options["datasets"]["train"]["batch_size"] == 3
    # main() gets past its argument parsing and stops where the GPU is needed (no fallback)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(AssertionError, match="MI355X"):
        fit.main(["stage1", "--root", "data", "--out", "run"])


def test_graph_is_refused_for_stage1(capsys):
    with pytest.raises(SystemExit) as ei:
        fit.parse_args(["stage1", "--root", "data", "--out", "run", "--graph"])
    assert ei.value.code == 2 and "--graph is not available for stage1" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--graph is not available for stage1"):
        fit.build_trainer("stage1", fit.default_options("stage1"), torch.device("cpu"), graph=True)
    assert fit.parse_args(["stage3", "--root", "data", "--out", "run", "--graph"])[0].graph          # the other stages keep it


def test_default_options_of_stage1():
    o = fit.default_options("stage1")
    d, tr = o["datasets"]["train"], o["train"]
    assert (d["GT_size"], d["batch_size"], d["use_flip"], d["use_crop"]) == (256, 4, True, True)
    assert (tr["beta1"], tr["beta2"]) == (0.5, 0.9)                                   # VQModel_arch.py:148-157
    assert tr["lr_G"] == 1e-4 and tr["codebook_weight"] == 1.0
    assert tr["lr_scheme"] == "MultiStepLR" and tr["lr_steps_rel"] == [0.5, 0.75, 0.9, 0.95] and tr["lr_gamma"] == 0.5 and tr["warmup_iter"] == 10
    assert o["logger"]["save_checkpoint_freq"] > 0 and o["logger"]["print_freq"] > 0
    other = fit.default_options("stage3")["train"]
    assert (other["beta1"], other["beta2"]) == (0.9, 0.99)                            # the other stages are untouched


def _stub_opt(lr=1e-4):
    scales = []
    groups = [types.SimpleNamespace(params=[], lr=lr, weight_decay=0.0), types.SimpleNamespace(params=[], lr=lr, weight_decay=0.0)]
    return types.SimpleNamespace(groups=groups, betas=(0.5, 0.9), eps=1e-8, t=0, set_lr_scale=scales.append, scales=scales,
                                 scaler_state_dict=lambda: dict(checkpoint.GRAD_SCALER_STATE), load_scaler_state_dict=lambda sd: None)


class _StubTrainer(train.Trainer):
    """Stage 1 as the driver sees it, built without a device: an optimizer, the network, and the tag of its checkpoint files."""

    checkpoint_tag = "VQ"

    def __init__(self, net):
        self.opt, self.netG = _stub_opt(), net


class _Stub:
    def __init__(self, out, net):
        self.trainer = _StubTrainer(net)
        self.out, self.steps = str(out), []

    def __len__(self):
        return 9

    def batch(self, indices):
        return tuple(indices), None

    def step(self, gt, lq):
        assert lq is None
        self.steps.append(gt)
        return torch.tensor(float(len(self.steps)))

    def run(self, niter, resume=None):
        o = fit.default_options("stage1")
        o["train"]["niter"], o["logger"]["save_checkpoint_freq"], o["logger"]["print_freq"] = niter, 4, 2
        recs = []
        fit.fit(o, self.trainer, self, self.out, step_fn=self.step, batch_fn=self.batch, log=recs.append, resume=resume)
        return recs


def test_stub_run_writes_vq_checkpoints_that_load_strictly_and_resumes(tmp_path):
    net = M.VQModel(ch=32, n_embed=64)
    a = _Stub(tmp_path, net)
    recs = a.run(10)
    assert len(a.steps) == 10 and recs[-1]["done"] and recs[-1]["last_checkpoint"] == 10
    assert a.trainer.opt.betas == (0.5, 0.9)                                          # the stage's betas reach the optimizer
    assert sorted(os.listdir(tmp_path / "models")) == sorted("%d_VQ.pth" % i for i in (4, 8, 10))
    assert sorted(os.listdir(tmp_path / "training_state")) == sorted("%d.state" % i for i in (4, 8, 10))
    # the file is a plain state dict under the VQModel key names: what --net-vq of stages 2 and 3, evaluate and enhance load
    sd = torch.load(tmp_path / "models" / "8_VQ.pth", map_location="cpu")
    assert set(sd) == set(net.state_dict()) and "quantize.embedding.weight" in sd and "post_quant_conv.weight" in sd
    fresh = M.VQModel(ch=32, n_embed=64)
    res = checkpoint.load_network(str(tmp_path / "models" / "8_VQ.pth"), fresh, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, fresh.state_dict()[k]) for k, v in net.state_dict().items())
    st = torch.load(tmp_path / "training_state" / "8.state", map_location="cpu", weights_only=False)
    assert st["iter"] == 8 and st["optimizers"][0]["param_groups"][0]["betas"] == (0.5, 0.9)
    # resume continues the iteration count, and the index sequence of the uninterrupted run
    b = _Stub(tmp_path, fresh)
    recs = b.run(10, resume=str(tmp_path / "training_state" / "8.state"))
    assert len(b.steps) == 2 and recs[-1]["iter"] == 10 and b.steps == a.steps[8:]


def test_never_used_list_is_exactly_the_parameters_without_a_gradient():
    """STAGE1_NEVER_USED by name against autograd of the CPU oracle's stage-1 graph (encoder -> quant_conv -> codebook with the
    straight-through form -> post_quant_conv -> decoder, L1 + qloss) at a small width: the parameter names are the product's."""
    from oracle import torch_ref as O

    ref = O.VQModel(ch=32, n_embed=64)
    assert set(dict(ref.named_parameters())) == set(dict(M.VQModel(ch=32, n_embed=64).named_parameters()))
    x = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(0))
    dec, qloss, _ = ref.decode(ref.encode(x)[0])
    ((dec - x).abs().mean() + qloss).backward()
    no_grad = sorted(n for n, p in ref.named_parameters() if p.grad is None)
    listed = sorted(n for n, _ in ref.named_parameters() if n.startswith(STAGE1_NEVER_USED))
    assert listed == no_grad == ["conv_semantic.0.bias", "conv_semantic.0.weight"]
