"""CPU: the averaged weights (--weights-ema) up to the device -- the option and its refusals, the checkpoint names and which sweep of
glare_amd.evaluate takes them, the two entry points of the ABI with the returns that need no launch, and the oracle's bound
(tests/weight_ema_fp64.py) exercised on an fp32 replay of the kernel's arithmetic."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import weight_ema_fp64 as W
from glare_amd import _lib, evaluate, fit, train, train_ops

DECAYS = (0.0, 0.5, 0.999, 0.9999)
SYMBOLS = ("glare_weight_ema_f32", "glare_swap_f32")


def _args(*extra, stage="stage3"):
    return fit.parse_args([stage, "--root", "data", "--out", "run"] + list(extra))[0]


@pytest.mark.parametrize("stage", ["stage1", "stage2", "stage3"])
def test_the_flag_parses_in_every_stage(stage):
    assert _args(stage=stage).weights_ema is None
    assert _args("--weights-ema", "0.999", stage=stage).weights_ema == 0.999
    assert _args("--weights-ema", "0", stage=stage).weights_ema == 0.0
    if stage != "stage1":
        assert _args("--weights-ema", "0.9", "--graph", stage=stage).graph
    else:
        a = _args("--weights-ema", "0.9", "--gan", "--codebook-ema", "0.99", "--codebook-restart", "10", stage=stage)
        assert a.gan and a.codebook_ema == 0.99 and a.weights_ema == 0.9


@pytest.mark.parametrize("value", ["1", "1.5", "-0.1", "nan"])
def test_a_decay_outside_the_range_is_refused_at_parse_time(value, capsys):
    with pytest.raises(SystemExit):
        _args("--weights-ema=" + value)
    assert "--weights-ema takes the decay of the moving average of the trained weights, a number in [0, 1) such as 0.999, not" in capsys.readouterr().err
    with pytest.raises(ValueError) as ei:
        fit.check_weights_ema_option(float(value))
    assert str(ei.value) == fit.WEIGHTS_EMA_REFUSAL % (float(value),)


def test_the_refusal_texts():
    assert fit.WEIGHTS_EMA_REFUSAL == ("--weights-ema takes the decay of the moving average of the trained weights, a number in [0, 1) such as "
                                       "0.999, not %r")
    assert train.EMA_RESUME_REFUSAL.startswith("--weights-ema: %s does not exist: a resumed run continues the average from the file written "
                                               "beside the weights")
    assert train.EMA_UNSEEDED_REFUSAL == "ema_weights(): no step has seeded the average yet (it starts as the weights after the first step)"
    assert evaluate.NO_EMA_FILES.startswith("--ema: %s holds no *_%s_ema.pth: the averaged weights are written by a run trained with")
    assert train.EMA_SUFFIX == "_ema" and train.WEIGHTS_EMA_KEY == "weights_ema"


@pytest.mark.parametrize("stage,tag", [("stage1", "VQ"), ("stage3", "G")])
def test_evaluate_takes_one_set_of_files_or_the_other(tmp_path, stage, tag):
    models = tmp_path / "models"
    models.mkdir()
    for it in (2, 10, 4):
        for suffix in ("", "_ema"):
            (models / ("%d_%s%s.pth" % (it, tag, suffix))).write_bytes(b"")
    (models / "4_D.pth").write_bytes(b"")
    names = lambda files: [os.path.basename(f) for f in files]
    assert names(evaluate.list_checkpoints(str(tmp_path), stage)) == ["%d_%s.pth" % (it, tag) for it in (2, 4, 10)]
    assert names(evaluate.list_checkpoints(str(tmp_path), stage, ema=True)) == ["%d_%s_ema.pth" % (it, tag) for it in (2, 4, 10)]


def test_evaluate_ema_without_such_files_says_so(tmp_path, capsys):
    (tmp_path / "models").mkdir()
    (tmp_path / "models" / "2_G.pth").write_bytes(b"")
    with pytest.raises(SystemExit):
        evaluate.main(["stage3", "--run", str(tmp_path), "--root", str(tmp_path), "--ema"])
    assert "holds no *_G_ema.pth" in capsys.readouterr().err


def test_a_trainer_without_the_option_has_no_second_network():
    """The interface's defaults, without a device: nothing more is written, nothing more recorded."""
    tr = train.Trainer.__new__(train.Trainer)
    assert tr.weights_ema is None and tr.extra_networks() == {} and tr.extra_state() == {} and not tr.ema_seeded()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return set(re.findall(r"\bT (glare_[a-z0-9_]+)", out))


def test_both_entry_points_are_declared_and_built_into_both_libraries():
    sigs = _lib.signatures()
    for name in SYMBOLS:
        assert name in sigs and name in _exports(_lib.LIB_PATH) and name in _exports(_lib.LIB_F16_PATH), name
    assert len(sigs["glare_weight_ema_f32"][1]) == 7 and len(sigs["glare_swap_f32"][1]) == 4
    assert _lib.main_lib().glare_version() >= 130
    header = open(_lib.HEADER_PATH).read()
    assert "basicsr/models/base_model.py:85-92" in header


def test_returns_that_need_no_launch():
    """Every refusal comes before a launch, so it holds without a device: n < 0, a null or misaligned pointer with n > 0, a decay outside
    [0, 1), ranges that overlap; n == 0 is a no-op whatever the pointers."""
    lib = _lib.main_lib()
    buf = _lib.host_f32([0.0] * 64)
    base = ctypes.addressof(buf)
    base += -base % 16
    a, b, flag = base, base + 64, base + 192
    ema = lambda *args: lib.glare_weight_ema_f32(*args, None)
    assert ema(a, b, 0, 0.5, 0.5, flag) == 0 and ema(None, None, 0, 0.5, 0.5, None) == 0
    assert ema(a, b, -1, 0.5, 0.5, flag) == _lib.ERR_INVALID
    for bad in (1.0, 1.5, -0.25, float("nan"), float("inf")):
        assert ema(a, b, 8, bad, 0.5, flag) == _lib.ERR_INVALID, bad
        assert ema(a, b, 0, bad, 0.5, flag) == _lib.ERR_INVALID, bad
    for args in ((None, b, 8, 0.5, 0.5, flag), (a, None, 8, 0.5, 0.5, flag), (a, b, 8, 0.5, 0.5, None), (a + 2, b, 8, 0.5, 0.5, flag),
                 (a, b + 1, 8, 0.5, 0.5, flag)):
        assert ema(*args) == _lib.ERR_INVALID, args
    swap = lambda *args: lib.glare_swap_f32(*args, None)
    assert swap(a, b, 0) == 0 and swap(None, None, 0) == 0 and swap(a, a, 0) == 0
    assert swap(a, b, -1) == _lib.ERR_INVALID
    for args in ((None, b, 8), (a, None, 8), (a + 2, b, 8), (a, b + 3, 8), (a, a, 8), (a, a + 4, 2), (a + 28, a, 8), (a, a + 28, 8)):
        assert swap(*args) == _lib.ERR_INVALID, args


def test_wrappers_refuse_cpu_tensors():
    e, w, flag = torch.zeros(8), torch.zeros(8), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        train_ops.weight_ema_(e, w, 0.9, flag)
    with pytest.raises(NotImplementedError):
        train_ops.swap_(e, w)


@pytest.mark.parametrize("decay", DECAYS)
def test_the_bound_holds_for_the_arithmetic_it_counts(decay):
    """10^6 random elements per decay, magnitudes over 24 binades and both signs: the fp32 replay of the kernel's three roundings stays
    inside the bound, and uses a good part of it (a bound nothing comes near would pin nothing)."""
    rng = np.random.default_rng(int(decay * 1e4) + 5)
    n = 10 ** 6
    mag = lambda: (rng.standard_normal(n) * np.exp2(rng.integers(-12, 12, n))).astype(np.float32)
    ema, w = mag(), mag()
    got = W.step_f32(ema, w, decay)
    ratio = np.abs(got.astype(np.float64) - W.rule(ema, w, decay)) / W.bound(ema, w, decay)
    print("decay %g: max |error| / bound = %.4f" % (decay, ratio.max()))
    assert ratio.max() <= 1.0
    if decay == 0.0:           # d = 0 keeps nothing of the old average, exactly
        assert np.array_equal(got, w)
    else:
        assert ratio.max() >= 0.1


def test_the_oracle_uses_the_decay_the_kernel_receives():
    assert W.f32(0.999) == float(np.float32(0.999)) != 0.999
    e, w = np.float32([1.0]), np.float32([3.0])
    assert W.rule(e, w, 0.5)[0] == 2.0 and W.bound(e, w, 0.5)[0] == 4 * 2.0 ** -24 * 2.0 + 2.0 ** -149
    assert list(W.classes(np.float32([np.nan, np.inf, -np.inf, 1.0, -1.0, 0.0, -0.0, 1e-40, -1e-40]))) == [0, 1, -1, 2, -2, 3, -3, 3, -3]
