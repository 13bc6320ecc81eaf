"""MI355X: the two kernels of csrc/weight_ema.hip per element -- the weight average against the fp64 rule and its derived one-step bound
(tests/weight_ema_fp64.py), the exchange bit for bit -- at every size where the code takes another path (fewer elements than a vector, the
scalar head and tail, one workgroup and several), with both pointers offset by 0..3 elements from a 16-byte boundary independently, guard
elements on both sides of every range, and +-0, a subnormal, +-inf and NaN planted in the weights.
Measured on an MI355X: the largest |error| / bound is 0.36 at every size up to 4097 and 0.39 at 4 x 65536 + 3."""
import numpy as np
import pytest
import torch

import weight_ema_fp64 as W
from glare_amd import _lib
from glare_amd import train_ops as T
from tolerances import within

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 4097, 4 * 65536 + 3]
DECAYS = [0.0, 0.5, 0.999, 0.9999]
GUARD = 8                                     # elements before and after a range (the base stays 16-byte aligned: 32 bytes)
SPECIALS = np.array([0.0, -0.0, 1e-40, np.inf, -np.inf, np.nan], dtype=np.float32)
PLANTED_EMA = np.array([0.0, -0.0, 0.0, 1.0, 1.0, 1.0], dtype=np.float32)      # what the average holds where a special weight sits


def _dev():
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _padded(values, off, seed):
    """values [n] inside a host buffer: GUARD + off elements of a recognisable pattern before, GUARD + (3 - off) after."""
    rng = np.random.default_rng(seed)
    full = rng.standard_normal(len(values) + 2 * GUARD + 3).astype(np.float32) + 100.0
    full[GUARD + off:GUARD + off + len(values)] = values
    return full


def _range(buf, off, n):
    t = buf[GUARD + off:GUARD + off + n]
    assert buf.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 4 * off and t.is_contiguous()
    return t


def _guards_hold(after, before, off, n):
    lo, hi = GUARD + off, GUARD + off + n
    return np.array_equal(_bits(after[:lo]), _bits(before[:lo])) and np.array_equal(_bits(after[hi:]), _bits(before[hi:]))


def _inputs(n):
    rng = np.random.default_rng(n)
    ema = (rng.standard_normal(n) * np.exp2(rng.integers(-6, 6, n))).astype(np.float32)
    w = (rng.standard_normal(n) * np.exp2(rng.integers(-6, 6, n))).astype(np.float32)
    k = min(n, len(SPECIALS))
    pos = np.unique(np.linspace(0, n - 1, k).astype(np.int64))
    w[pos], ema[pos] = SPECIALS[:len(pos)], PLANTED_EMA[:len(pos)]
    return ema, w, pos


@pytest.mark.parametrize("n", SIZES)
def test_weight_ema_per_element(n):
    ema, w, pos = _inputs(n)
    flags = {v: torch.full((1,), v, dtype=torch.int32, device=_dev()) for v in (0, 1)}
    worst = 0.0
    for ow in range(4):
        w_host = _padded(w, ow, 1)
        w_buf = torch.from_numpy(w_host).to(_dev())
        for oe in range(4):
            e_host = _padded(ema, oe, 2)
            for decay in DECAYS:
                exact, bound = W.rule(ema, w, decay), W.bound(ema, w, decay)
                finite = np.isfinite(exact)
                for seeded in (0, 1):
                    e_buf = torch.from_numpy(e_host).to(_dev())
                    T.weight_ema_(_range(e_buf, oe, n), _range(w_buf, ow, n), decay, flags[seeded])
                    after = e_buf.cpu().numpy()
                    got = after[GUARD + oe:GUARD + oe + n]
                    tag = (n, oe, ow, decay, seeded)
                    assert _guards_hold(after, e_host, oe, n), tag
                    if not seeded:
                        assert np.array_equal(_bits(got), _bits(w)), tag            # the seed: a bit copy, NaN payload and -0 included
                        continue
                    assert np.array_equal(W.classes(got), W.classes(exact)), (tag, got[pos], exact[pos])
                    worst = max(worst, float((np.abs(got[finite].astype(np.float64) - exact[finite]) / bound[finite]).max()))
        assert np.array_equal(_bits(w_buf.cpu().numpy()), _bits(w_host)), (n, ow)   # the weights are only read
        assert int(flags[0]) == 0 and int(flags[1]) == 1                            # ... and so is the flag
    print("n = %d: max |error| / bound = %.4f" % (n, worst))
    within(worst, 1.0, "n=%d" % n)


@pytest.mark.parametrize("n", SIZES)
def test_swap_is_bit_exact_and_its_own_inverse(n):
    a, b, _ = _inputs(n)
    b = b[::-1].copy()
    for oa in range(4):
        for ob in range(4):
            a_host, b_host = _padded(a, oa, 3), _padded(b, ob, 4)
            a_buf, b_buf = torch.from_numpy(a_host).to(_dev()), torch.from_numpy(b_host).to(_dev())
            T.swap_(_range(a_buf, oa, n), _range(b_buf, ob, n))
            a1, b1 = a_buf.cpu().numpy(), b_buf.cpu().numpy()
            assert np.array_equal(_bits(a1[GUARD + oa:GUARD + oa + n]), _bits(b)), (n, oa, ob)
            assert np.array_equal(_bits(b1[GUARD + ob:GUARD + ob + n]), _bits(a)), (n, oa, ob)
            assert _guards_hold(a1, a_host, oa, n) and _guards_hold(b1, b_host, ob, n), (n, oa, ob)
            T.swap_(_range(a_buf, oa, n), _range(b_buf, ob, n))
            assert np.array_equal(_bits(a_buf.cpu().numpy()), _bits(a_host)) and np.array_equal(_bits(b_buf.cpu().numpy()), _bits(b_host))


def test_refusals_on_device_pointers():
    """n < 0, a null pointer with n > 0, a decay outside [0, 1), ranges that overlap: GLARE_ERR_INVALID and nothing written; n == 0 returns 0."""
    lib = _lib.main_lib()
    buf = torch.arange(64, dtype=torch.float32, device=_dev())
    before = buf.clone()
    flag = torch.ones(1, dtype=torch.int32, device=_dev())
    a, b, f, st = buf.data_ptr(), buf.data_ptr() + 128, flag.data_ptr(), _lib.stream_handle()
    assert lib.glare_weight_ema_f32(a, b, 0, 0.5, 0.5, f, st) == 0 and lib.glare_swap_f32(a, b, 0, st) == 0
    assert lib.glare_weight_ema_f32(a, b, -1, 0.5, 0.5, f, st) == _lib.ERR_INVALID and lib.glare_swap_f32(a, b, -1, st) == _lib.ERR_INVALID
    for bad in (1.0, 2.0, -0.5, float("nan")):
        assert lib.glare_weight_ema_f32(a, b, 16, bad, 0.5, f, st) == _lib.ERR_INVALID, bad
    for args in ((None, b, 16, 0.5, 0.5, f), (a, None, 16, 0.5, 0.5, f), (a, b, 16, 0.5, 0.5, None)):
        assert lib.glare_weight_ema_f32(*args, st) == _lib.ERR_INVALID, args
    for args in ((None, b, 16), (a, None, 16), (a, a, 16), (a, a + 4, 16), (a + 60, a, 16), (a, a + 60, 16)):
        assert lib.glare_swap_f32(*args, st) == _lib.ERR_INVALID, args
    assert lib.glare_swap_f32(a, a + 64, 16, st) == 0                       # adjacent ranges do not overlap
    with pytest.raises(_lib.GlareError) as ei:
        T.swap_(buf[0:16], buf[8:24])
    assert ei.value.status == _lib.ERR_INVALID
    with pytest.raises(_lib.GlareError) as ei:
        T.weight_ema_(buf[0:16], buf[32:48], 1.0, flag)
    assert ei.value.status == _lib.ERR_INVALID
    torch.cuda.synchronize()
    expect = before.clone()
    expect[0:16], expect[16:32] = before[16:32], before[0:16]               # the one exchange that was valid
    assert torch.equal(buf, expect)
