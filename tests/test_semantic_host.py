"""CPU: the semantic guidance term's fp64 restatement (tests/semantic_fp64.py) against torch autograd of the oracle's conv_semantic, the
strict VGG19 loader, the C entries' refusals, and the option surface of the driver and the trainer.  Every test names something the
parent commit lacks (losses.load_vgg19, fit.check_semantic_options, the glare_vq_semantic_* entries, Stage1Trainer's semantic term)."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

import semantic_fp64 as S
from glare_amd import _lib, fit, losses, train


@pytest.mark.parametrize("n_tokens,seed", [(1, 0), (64, 1), (2 * 5 * 7, 2)])
def test_restatement_equals_autograd_of_the_oracle_branch(n_tokens, seed):
    """loss, dq, dW, db of the helper against fp64 autograd of F.mse_loss(conv_semantic(quant), feat) with oracle.torch_ref's module, on
    the grid inputs: channel 5 (W = 0, b = 0) and token 0 of every channel with b = 0 have a pre-activation of exactly 0."""
    from oracle import torch_ref as O

    q, W, b, feat = S.grid_case(n_tokens, seed, torch.float16)
    conv = O.VQModel().conv_semantic.double()
    with torch.no_grad():
        conv[0].weight.copy_(W.double().view(256, 3, 1, 1))
        conv[0].bias.copy_(b.double())
    quant = q.double().t().reshape(1, 3, n_tokens, 1).clone().requires_grad_(True)           # NCHW, one token per row
    target = feat.double().t().reshape(1, 256, n_tokens, 1)
    pre = F.conv2d(quant.detach(), conv[0].weight, conv[0].bias)
    assert int((pre == 0).sum()) >= n_tokens                                                  # exact zeros are part of the case
    loss = F.mse_loss(conv(quant), target)
    loss.backward()
    got = S.semantic(q, W, b, feat)
    want = (loss.detach(), quant.grad.reshape(3, n_tokens).t(), conv[0].weight.grad.view(256, 3), conv[0].bias.grad)
    for name, a, r in zip(("loss", "dq", "dW", "db"), got, want):
        assert a.shape == r.shape, name
        assert float((a - r).abs().max()) <= 1e-14 * max(1.0, float(r.abs().max())), name
    assert float(got[2][5].abs().max()) == 0.0 and float(got[3][5]) == 0.0 and float(got[3][9]) == 0.0     # 0 at pre == 0; dead channel


def test_geometry_and_bounds_of_the_kernel_model():
    assert S.geometry(1) == (1, 1, 1) and S.geometry(64) == (1, 64, 16) and S.geometry(65) == (2, 33, 9)
    assert S.geometry(5003) == (79, 64, 16) and S.geometry(512 * 64) == (512, 64, 16) and S.geometry(512 * 64 + 1) == (505, 65, 17)
    q, W, b, feat = S.grid_case(65, 3, torch.bfloat16)
    exact, general = S.bounds(q, W, b, feat, pre_roundings=0), S.bounds(q, W, b, feat)
    for a, g in zip(exact, general):
        assert bool((a <= g).all()) and bool((a >= 0).all())
    assert float(exact[2][5].abs().max()) == 0.0 and float(exact[3][9]) == 0.0               # nothing is added: the bound is 0


def test_load_vgg19_takes_both_key_forms_and_refuses_by_name():
    net = losses.SemanticTarget()
    assert [n for n, _ in net.named_parameters()] == ["features.%d.%s" % (i, t) for i, _, _ in S.VGG19_CONVS for t in ("weight", "bias")]
    assert not any(p.requires_grad for p in net.parameters()) and not net.train().training
    sd = S.seeded_vgg19(4, whole=True)
    keys = losses.load_vgg19(net, sd)
    assert len(keys) == 16 and all(torch.equal(net.state_dict()[k], sd[k]) for k in keys)
    other = losses.SemanticTarget()
    assert losses.load_vgg19(other, S.seeded_vgg19(4, form="vgg_net", whole=True)) == keys
    assert all(torch.equal(a, b) for a, b in zip(net.parameters(), other.parameters()))
    with pytest.raises(ValueError) as e:
        losses.load_vgg19(losses.SemanticTarget(), S.vgg16_shaped())
    assert "features.16.weight" in str(e.value) and "features.16.bias" in str(e.value) and "features.14" not in str(e.value)
    short = {k: v for k, v in S.seeded_vgg19(4).items() if k != "features.7.bias"}
    with pytest.raises(ValueError) as e:
        losses.load_vgg19(losses.SemanticTarget(), short)
    assert "features.7.bias" in str(e.value) and "features.7.weight" not in str(e.value)
    bent = dict(S.seeded_vgg19(4), **{"features.10.weight": torch.zeros(256, 64, 3, 3)})
    with pytest.raises(ValueError, match=r"features\.10\.weight: \(256, 64, 3, 3\) in the file"):
        losses.load_vgg19(losses.SemanticTarget(), bent)
    with pytest.raises(ValueError):
        losses.load_vgg19(losses.SemanticTarget(), None)


def test_semantic_target_refuses_sizes_and_cpu_tensors():
    net = losses.SemanticTarget()
    with pytest.raises(ValueError, match="multiples of 4"):
        net(torch.zeros(2, 66, 64, 3))
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 8, 8, 3))


def test_options_are_refused_before_anything_is_built(capsys):
    for stage in ("stage2", "stage3"):
        for kw in ({"vgg19": "v.pth"}, {"semantic_weight": 0.1}):
            with pytest.raises(ValueError) as e:
                fit.check_semantic_options(stage, **kw)
            assert str(e.value) == fit.SEMANTIC_REFUSAL
            with pytest.raises(ValueError) as e:
                fit.build_trainer(stage, fit.default_options(stage), "cpu", **kw)
            assert str(e.value) == fit.SEMANTIC_REFUSAL
        with pytest.raises(SystemExit):
            fit.parse_args([stage, "--root", "x", "--out", "y", "--vgg19", "v.pth"])
        assert "--vgg19 / --semantic-weight are stage1 options" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--semantic-weight needs --vgg19"):
        fit.check_semantic_options("stage1", None, 0.2)
    with pytest.raises(ValueError, match="--semantic-weight needs --vgg19"):
        fit.build_trainer("stage1", fit.default_options("stage1"), "cpu", semantic_weight=0.2)
    with pytest.raises(SystemExit):
        fit.parse_args(["stage1", "--root", "x", "--out", "y", "--semantic-weight", "0.2"])
    assert "--semantic-weight needs --vgg19" in capsys.readouterr().err
    fit.check_semantic_options("stage1")
    fit.check_semantic_options("stage1", "v.pth", 0.2)
    fit.check_semantic_options("stage3")
    args, _ = fit.parse_args(["stage1", "--root", "x", "--out", "y", "--vgg19", "v.pth", "--semantic-weight", "0.2"])
    assert args.vgg19 == "v.pth" and args.semantic_weight == 0.2
    args, _ = fit.parse_args(["stage1", "--root", "x", "--out", "y"])
    assert args.vgg19 is None and args.semantic_weight is None


def test_objective_tag_names_the_term_and_its_weight():
    tag = train.Stage1Trainer.objective_tag
    me = lambda **kw: types.SimpleNamespace(**dict({"perceptual": None, "perceptual_weight": 1.0, "semantic": None, "semantic_weight": 0.1}, **kw))
    sem = losses.SemanticTarget()
    assert tag(me()) is None
    assert tag(me(semantic=sem)) == "SemanticTarget x 0.1"
    assert tag(me(semantic=sem, semantic_weight=0.2)) == "SemanticTarget x 0.2" != tag(me(semantic=sem))
    both = tag(me(semantic=sem, perceptual=losses.LPIPSLoss(), perceptual_weight=2.0))
    assert both == "LPIPSLoss x 2 + SemanticTarget x 0.1" and tag(me(perceptual=losses.LPIPSLoss())) == "LPIPSLoss x 1"
    assert train.STAGE1_NEVER_USED == ("conv_semantic.",) and train.SEMANTIC_TERMS == ("semantic_loss",)


def test_train_nhwc_refuses_a_feature_map_of_another_size_before_any_launch():
    from glare_amd import modules as M

    net = M.VQModel()
    assert net.semantic_weight == 0.1
    for x, feat in ((torch.zeros(2, 3, 64, 64), torch.zeros(2, 16, 15, 256)), (torch.zeros(2, 3, 66, 64), torch.zeros(2, 16, 16, 256)),
                    (torch.zeros(2, 3, 64, 64), torch.zeros(2, 16, 16, 128))):
        with pytest.raises(ValueError, match="vgg_feat"):              # (a CPU tensor would raise NotImplementedError at the first launch)
            net.train_nhwc(x, feat)
    with pytest.raises(AssertionError):
        net.decode(torch.zeros(1, 3, 4, 4), vgg_feat=torch.zeros(1))


def test_header_types_the_entries_and_they_refuse_before_launching():
    c = ctypes
    sigs = _lib.signatures()
    assert sigs["glare_vq_semantic_workspace_bytes"] == (c.c_size_t, [c.c_longlong, c.c_int])
    assert sigs["glare_vq_semantic_bf16"] == (c.c_int, [c.c_void_p] * 4 + [c.c_longlong, c.c_int] + [c.c_void_p] * 5 + [c.c_size_t, c.c_void_p])
    assert sigs["glare_vq_semantic_scale_f32"] == (c.c_int, [c.c_void_p, c.c_longlong] + [c.c_void_p] * 7)
    INV, UNS, WSP = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    for prec in ("bf16", "fp16"):
        with _lib.use_precision(prec):
            lib = _lib.lib()
            ws, f = lib.glare_vq_semantic_workspace_bytes, lib.glare_vq_semantic_bf16
            row = (3 * 256 + 256 + 4) * 4                             # a workgroup's partial row: dW | db | loss, padded to 16 bytes
            assert [ws(n, 256) for n in (1, 64, 65, 5003, 512 * 64, 512 * 64 + 1, 1 << 24)] == [row * g for g in (1, 1, 2, 79, 512, 505, 512)]
            assert ws(0, 256) == 0 and ws(-1, 256) == 0 and ws((1 << 24) + 1, 256) == 0 and ws(64, 128) == 0
            buf = (c.c_longlong * 64)()                               # host memory: every call below returns before it would be read
            p = c.addressof(buf)
            for i in (0, 1, 2, 3, 6, 7, 8, 9):                        # quant, weight, bias, feat, loss, dq, dW, db
                args = [p, p, p, p, 8, 256, p, p, p, p, p, 1 << 20, None]
                args[i] = None
                assert f(*args) == INV, i
            assert f(p, p, p, p, 0, 256, p, p, p, p, p, 1 << 20, None) == INV and f(p, p, p, p, -8, 256, p, p, p, p, p, 1 << 20, None) == INV
            assert f(p, p, p, p, 8, 0, p, p, p, p, p, 1 << 20, None) == INV
            assert f(p, p, p, p + 4, 8, 256, p, p, p, p, p, 1 << 20, None) == INV                      # feat is read 8 bytes at a time
            assert f(p, p, p, p, 8, 128, p, p, p, p, p, 1 << 20, None) == UNS
            assert f(p, p, p, p, (1 << 24) + 1, 256, p, p, p, p, p, 1 << 40, None) == UNS
            assert f(p, p, p, p, 8, 256, p, p, p, p, p, ws(8, 256) - 1, None) == WSP
            assert f(p, p, p, p, 70, 256, p, p, p, p, p, ws(70, 256) - 1, None) == WSP
            assert f(p, p, p, p, 8, 256, p, p, p, p, None, 1 << 20, None) == WSP
            assert not any(buf)
    g = _lib.main_lib().glare_vq_semantic_scale_f32
    assert g(None, 8, p, p, p, p, p, p, None) == INV and g(p, 0, p, p, p, p, p, p, None) == INV
    assert g(p, 8, None, p, p, p, p, p, None) == INV and g(p, 8, p, None, p, p, p, p, None) == INV
    assert g(p, (1 << 24) + 1, p, p, p, p, p, p, None) == UNS
    assert _lib.main_lib().glare_version() >= 129


def test_ops_refuse_cpu_tensors():
    from glare_amd import ops

    with pytest.raises(NotImplementedError):
        ops.vq_semantic(torch.zeros(4, 3), torch.zeros(256, 3), torch.zeros(256), torch.zeros(4, 256, dtype=torch.bfloat16))
    with pytest.raises(NotImplementedError):
        ops.vq_semantic_scale(torch.ones(1), torch.zeros(4, 3), torch.zeros(256, 3), torch.zeros(256))
