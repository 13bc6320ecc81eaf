"""MI355X: --weights-ema through the training driver -- stage 3 on the synthetic folders of tests/test_gpu_fit.py (6 pairs, 2 x 256^2
crops, name-seeded nets), niter 4, a checkpoint every 2 steps, eager and --graph, and a resume from step 2.

The yardstick of every closeness claim is what the run's own weights do: the average is a convex combination of the weights of the
steps so far, so two runs' averages can differ by no more than their weights did at some step up to there, plus the average's own
roundings (4 U max |w| per step, tests/weight_ema_fp64.py).
Measured on an MI355X: eager against --graph, and resumed against uninterrupted, differ by 0 in the weights and by 0 in the average."""
import json
import os

import numpy as np
import pytest
import torch

import weight_ema_fp64 as W
from glare_amd import fit, train

pytestmark = pytest.mark.gpu

DECAY = 0.9
COMMON = ["--niter", "4", "--save-freq", "2", "--weights-ema", str(DECAY)]


def _write(folder, name, h, w, rng):
    from PIL import Image

    os.makedirs(folder, exist_ok=True)
    Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(folder, name))


def _make_v1(root, split, sizes, seed):
    rng = np.random.default_rng(seed)
    for i, (h, w) in enumerate(sizes):
        _write(os.path.join(root, split, "low"), "%02d.png" % i, h, w, rng)
        _write(os.path.join(root, split, "high"), "%02d.png" % i, h, w, rng)


def _run(root, out, tmp, *extra):
    opt = os.path.join(str(tmp), "opt.json")
    with open(opt, "w") as f:
        json.dump({"logger": {"print_freq": 1}}, f)
    return fit.main(["stage3", "--root", root, "--out", out, "--opt", opt] + COMMON + list(extra))


def _load(out, name):
    return torch.load(os.path.join(out, "models", name), map_location="cpu")


def _max_diff(a, b, keys):
    return max(float((a[k].double() - b[k].double()).abs().max()) for k in keys)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("weights_ema")
    root = str(tmp / "data")
    _make_v1(root, "our485", [(260, 300), (256, 256), (300, 270), (272, 401), (257, 263), (288, 256)], seed=1)
    _make_v1(root, "eval15", [(44, 76)] * 3, seed=2)
    res = {"root": root, "tmp": tmp}
    for name, extra in (("eager", []), ("graph", ["--graph"])):
        res[name] = str(tmp / name)
        res[name + "_records"] = _run(root, res[name], tmp, *extra)
    return res


def _trained(sd):
    return [k for k in sd if k.startswith("deformable_decoder.") and not k.startswith(train.STAGE3_NEVER_USED)]


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_every_checkpoint_has_the_averaged_file(runs, mode):
    out = runs[mode]
    w2, w4 = _load(out, "2_G.pth"), _load(out, "4_G.pth")
    for it in (2, 4):
        live, avg = (w2 if it == 2 else w4), _load(out, "%d_G_ema.pth" % it)
        assert list(avg) == list(live)
        trained = _trained(live)
        assert trained and len(trained) < len(live)
        rest = [k for k in live if k not in set(trained)]
        assert all(torch.equal(avg[k], live[k]) for k in rest)
        assert all(avg[k].dtype == live[k].dtype and avg[k].shape == live[k].shape for k in live)
        # the average differs from the weights on every trained tensor -- that trains: one whose gradient is zero stands still under Adam
        # (its file entries at 2 and 4 are equal), and the average of a constant is the constant
        still = [k for k in trained if torch.equal(avg[k], live[k])]
        print("%s iter %d: %d trained tensors, %d equal to their average" % (mode, it, len(trained), len(still)))
        assert all(torch.equal(w2[k], w4[k]) for k in still), still
        assert len(still) < len(trained)
    records = runs[mode + "_records"]
    last = records[-2]
    assert last["iter"] == 4 and set(last["val_ema"]) == set(last["val"]) == {"images", "psnr", "ssim"}
    assert last["val_ema"]["images"] == 3 and np.isfinite(last["val_ema"]["psnr"]) and np.isfinite(last["val_ema"]["ssim"])
    assert last["val_ema"] != last["val"]
    st = torch.load(os.path.join(out, "training_state", "4.state"), map_location="cpu", weights_only=False)
    assert st[train.WEIGHTS_EMA_KEY] == {"decay": DECAY}


def _average_slack(sd, keys):
    return 4 * W.ROUNDINGS * W.U * max(float(sd[k].abs().max()) for k in keys)      # four steps of the average's own roundings


def test_eager_and_graph_averages_agree_as_their_weights_do(runs):
    worst_g = 0.0
    for it in (2, 4):
        ge, gg = _load(runs["eager"], "%d_G.pth" % it), _load(runs["graph"], "%d_G.pth" % it)
        ee, eg = _load(runs["eager"], "%d_G_ema.pth" % it), _load(runs["graph"], "%d_G_ema.pth" % it)
        keys = _trained(ge)
        d_g, d_e = _max_diff(ge, gg, keys), _max_diff(ee, eg, keys)
        worst_g = max(worst_g, d_g)
        print("iter %d: eager-vs-graph max |diff|: weights %.3g, averaged %.3g" % (it, d_g, d_e))
        assert d_e <= worst_g + _average_slack(ge, keys), (it, d_e, worst_g)


def test_a_resumed_run_continues_the_average(runs):
    import shutil

    out = str(runs["tmp"] / "resumed")
    os.makedirs(os.path.join(out, "models"))
    os.makedirs(os.path.join(out, "training_state"))
    for name in ("2_G.pth", "2_G_ema.pth"):
        shutil.copy(os.path.join(runs["eager"], "models", name), os.path.join(out, "models", name))
    state = os.path.join(out, "training_state", "2.state")
    shutil.copy(os.path.join(runs["eager"], "training_state", "2.state"), state)
    records = _run(runs["root"], out, runs["tmp"], "--resume", state)
    assert [r["iter"] for r in records[:-1]] == [3, 4] and "val_ema" in records[-2]
    g0, g1 = _load(runs["eager"], "4_G.pth"), _load(out, "4_G.pth")
    e0, e1 = _load(runs["eager"], "4_G_ema.pth"), _load(out, "4_G_ema.pth")
    keys = _trained(g0)
    d_g, d_e = _max_diff(g0, g1, keys), _max_diff(e0, e1, keys)
    print("resumed-vs-uninterrupted at iter 4, max |diff|: weights %.3g, averaged %.3g" % (d_g, d_e))
    assert d_e <= d_g + _average_slack(g0, keys), (d_e, d_g)
    assert not all(torch.equal(e1[k], g1[k]) for k in keys)                          # an average, not a re-seeded copy of the weights

    # the same resume with the averaged file gone is refused, and the refusal names the file
    gone = os.path.join(out, "models", "2_G_ema.pth")
    os.remove(gone)
    with pytest.raises(ValueError) as ei:
        _run(runs["root"], out, runs["tmp"], "--resume", state)
    assert str(ei.value) == train.EMA_RESUME_REFUSAL % gone
