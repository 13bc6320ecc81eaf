"""MI355X: the weight average inside the optimizer and the trainers (train.FlatAdam / train.Trainer, weights_ema=): every step against the
one-step oracle (tests/weight_ema_fp64.py) applied to the DEVICE's previous average -- so nothing accumulates and the one-step bound
applies --, the averaged state dict, the exchange context, training left untouched by the option, and a hipGraph capture that neither
seeds nor advances the average.
Measured on an MI355X: |error| / bound 0.43-0.46 per step (a skipped step and a graph replay included); off-vs-off and on-vs-off are 0 in
loss, weights and moments."""
import numpy as np
import pytest
import torch

import weight_ema_fp64 as W
from tolerances import within

pytestmark = pytest.mark.gpu

DECAY = 0.9


def _dev():
    return torch.device("cuda", 0)


def _trainer(seed=6, **kw):
    """The 2 x 64^2 Stage1Trainer of tests/test_gpu_stage1.py (fp16, at a scale no step of the toy problem overflows at)."""
    from glare_amd import modules as M
    from glare_amd.synthetic import seeded_init_
    from glare_amd.train import Stage1Trainer

    tr = Stage1Trainer(seeded_init_(M.VQModel().train(), seed).to(_dev()), precision="fp16", **kw)
    tr.opt.scale.fill_(1024.0)
    return tr


def _batch(seed=31, B=2, S=64):
    return torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(seed)).to(_dev())


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _check_step(ema_before, ema_after, w_after, decay, tag):
    exact, bound = W.rule(ema_before.cpu().numpy(), w_after.cpu().numpy(), decay), W.bound(ema_before.cpu().numpy(), w_after.cpu().numpy(), decay)
    assert np.isfinite(exact).all(), tag
    ratio = float((np.abs(ema_after.cpu().numpy().astype(np.float64) - exact) / bound).max())
    print("%s: max |error| / bound = %.4f" % (tag, ratio))
    return within(ratio, 1.0, tag)


def test_every_step_follows_the_rule_and_the_trainer_serves_the_average():
    tr = _trainer(weights_ema=DECAY)
    g = tr.opt.groups[0]
    assert tr.weights_ema == DECAY and g.ema.shape == g.w.shape and g.ema.data_ptr() != g.w.data_ptr()
    assert not hasattr(tr.opt.groups[1], "ema")                                   # the empty second group gets none
    assert int(tr.opt.ema_seeded) == 0 and not tr.ema_seeded()
    live = tr.net.state_dict()
    before = tr.ema_state_dict()                                                  # before the first step: the live weights
    assert list(before) == list(live) and all(v.data_ptr() == live[k].data_ptr() for k, v in before.items())
    with pytest.raises(RuntimeError) as ei:
        with tr.ema_weights():
            pass
    from glare_amd import train

    assert str(ei.value) == train.EMA_UNSEEDED_REFUSAL
    x = _batch()
    for step in range(1, 5):
        ema_before = g.ema.clone()
        tr.step(x)
        assert not tr.opt.last_step_skipped()
        assert int(tr.opt.ema_seeded) == 1
        if step == 1:
            assert torch.equal(_bits(g.ema), _bits(g.w))                          # ema_1 = w_1, bit for bit
        else:
            assert not torch.equal(g.ema, g.w)
            _check_step(ema_before, g.ema, g.w, DECAY, "step %d" % step)
    # a step the GradScaler skips: the weights stay, the average goes on decaying toward them
    ema_before, w_before = g.ema.clone(), g.w.clone()
    tr.step_tensor(x * 1e6)
    assert tr.opt.last_step_skipped() and torch.equal(g.w, w_before)
    _check_step(ema_before, g.ema, g.w, DECAY, "skipped step")

    # the averaged state dict: the network's keys; a trained tensor is its slice of `ema`, anything else the live one
    live, avg = tr.net.state_dict(), tr.ema_state_dict()
    assert list(avg) == list(live)
    lo, hi = g.w.data_ptr(), g.w.data_ptr() + 4 * g.w.numel()
    elo = g.ema.data_ptr()
    never = {p.data_ptr() for p, used in zip(g.params, g.has_grad) if not used}
    n_avg = 0
    for k, v in live.items():
        if lo <= v.data_ptr() < hi and v.data_ptr() not in never:
            off = v.data_ptr() - lo
            assert avg[k].data_ptr() == elo + off and avg[k].shape == v.shape, k
            n_avg += 1
        else:
            assert avg[k].data_ptr() == v.data_ptr(), k
        if v.data_ptr() in never:       # never updated: the average of a constant, up to its roundings (4 U |w| a step, contracted by d)
            e = g.ema[(v.data_ptr() - lo) // 4:(v.data_ptr() - lo) // 4 + v.numel()]
            assert float((e - v.reshape(-1)).abs().max()) <= W.ROUNDINGS * W.U / (1 - DECAY) * float(v.abs().max()), k
    assert n_avg == sum(g.has_grad) and n_avg < len(live) and any(not torch.equal(avg[k], live[k]) for k in live)
    nets = tr.extra_networks()
    assert list(nets) == ["VQ_ema"] and list(nets["VQ_ema"].state_dict()) == list(live)
    assert tr.extra_state()[train.WEIGHTS_EMA_KEY] == {"decay": DECAY}

    # the exchange context: the averaged weights inside, everything bit-identical after
    tr.net.eval()
    w0, e0 = g.w.clone(), g.ema.clone()
    key0 = next(k for k in live if avg[k].data_ptr() != live[k].data_ptr())
    avg0 = avg[key0].clone()
    with torch.no_grad():
        z_live = tr.net.encode_nhwc(x).clone()
        with tr.ema_weights():
            assert not torch.equal(g.w, w0)
            assert torch.equal(_bits(tr.net.state_dict()[key0]), _bits(avg0))
            z_avg = tr.net.encode_nhwc(x).clone()
        z_again = tr.net.encode_nhwc(x)
    assert torch.equal(_bits(g.w), _bits(w0)) and torch.equal(_bits(g.ema), _bits(e0))
    assert not torch.equal(z_avg, z_live) and torch.equal(z_again, z_live)


def test_the_option_leaves_training_untouched():
    """Three trainers from one seed -- off, off, on -- three steps each: on-vs-off differs in loss and weights by no more than off-vs-off
    (expected 0: the step is deterministic; printed).  Off, nothing is allocated."""
    runs = []
    for kw in ({}, {}, {"weights_ema": DECAY}):
        tr = _trainer(**kw)
        x = _batch(33)
        losses = [tr.step(x) for _ in range(3)]
        runs.append((losses, tr.opt.groups[0].w.clone(), tr.opt.groups[0].m.clone()))
        if not kw:
            assert tr.weights_ema is None and tr.opt.ema_seeded is None and tr.opt.ema_tensors() == []
            assert not any(hasattr(g, "ema") for g in tr.opt.groups)
            assert tr.extra_networks() == {} and tr.extra_state() == {}
    dist = lambda a, b: (max(abs(p - q) for p, q in zip(a[0], b[0])), float((a[1] - b[1]).abs().max()), float((a[2] - b[2]).abs().max()))
    off_off, on_off = dist(runs[0], runs[1]), dist(runs[2], runs[0])
    print("off-vs-off (loss, w, exp_avg):", off_off, " on-vs-off:", on_off)
    assert all(a <= b for a, b in zip(on_off, off_off)), (on_off, off_off)


def test_a_graph_capture_neither_seeds_nor_advances_the_average():
    """Stage 3 at the sizes of tests/test_gpu_fit.py (2 x 256^2): GraphedStep's warm-up runs real steps and puts the state back -- the average
    and its flag included; the replays then seed it and follow the rule."""
    from glare_amd import fit, train

    options = fit.default_options("stage3")
    tr = fit.build_trainer("stage3", options, _dev(), weights_ema=DECAY)
    g = tr.opt.groups[0]
    gen = torch.Generator().manual_seed(5)
    gt = torch.rand(2, 3, 256, 256, generator=gen).to(_dev())
    lq = torch.log(torch.clamp(torch.rand(2, 3, 256, 256, generator=gen) * 0.2 + 1e-3, min=1e-3)).to(_dev())
    g.ema.copy_(torch.arange(g.ema.numel(), dtype=torch.float32, device=_dev()) * 0.5)      # recognisable, and nothing a step could write
    e0, w0 = g.ema.clone(), g.w.clone()
    graphed = train.GraphedStep(tr, gt, lq)
    assert int(tr.opt.ema_seeded) == 0 and torch.equal(_bits(g.ema), _bits(e0)) and torch.equal(_bits(g.w), _bits(w0))
    graphed.step(gt, lq)
    assert int(tr.opt.ema_seeded) == 1 and torch.equal(_bits(g.ema), _bits(g.w)) and not torch.equal(g.w, w0)
    ema_before = g.ema.clone()
    graphed.step(gt, lq)
    assert not torch.equal(g.ema, g.w)
    _check_step(ema_before, g.ema, g.w, DECAY, "replay 2")
