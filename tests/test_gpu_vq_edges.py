"""GPU: the codebook search (csrc/vq.hip, glare_vq_nearest_f32 behind ops.vq_nearest) in ALL THREE of its launch shapes -- 64 token lanes x 16
code ranges up to 32 768 tokens, 128 x 8 up to 65 536, 256 x 4 above -- on both sides of each switch, with a ragged last workgroup in each
(vq_fp64.SMALL_N / LARGE_N), at code counts that divide by the number of ranges, that do not, that are smaller than it (empty ranges), and
that leave one code for a second and a third resident chunk (vq_fp64.SMALL_K / LARGE_K).

Families (vq_fp64.FAMILIES, shown on the CPU to have the property each claims: test_vq_scoring_fp64_host.py): random; tokens at the
fp32-rounded midpoint of a code and its nearest neighbour at code scales 0.7 and 30 and with the codebook shifted off the origin (the oracle's
choice differs from the fp64 argmin for 4 tokens in 10: the documented sequence of roundings decides); duplicated code rows in different
ranges and in different resident chunks, the tokens equal to them (the lower index must win the merge); NaN and infinite tokens and NaN code
rows.  Every family is built once at the largest count and cut to length, so the oracle runs once per (family, K).

Asserted for every token of every case: idx and z_q equal the C oracle's bit for bit; z_q is codebook[idx] bit for bit; the fp64 distance of
the chosen code exceeds the fp64 minimum over ALL K codes by no more than C_ROUND U ((zz + ee_chosen) + (zz + ee_best)) (vq_fp64's header
counts C_ROUND = 8 from the kernel; computed on the device in fp64, independent of the oracle); two runs give the same bits; want_zq=False
gives the same indices; the buffers around idx and z_q keep their fill.  The refusals leave pre-filled outputs alone."""
import functools

import numpy as np
import pytest
import torch

import vq_fp64 as R
from glare_amd import _lib, ops
from glare_amd._lib import ptr, stream_handle
from tolerances import within

pytestmark = pytest.mark.gpu

N_MAX = max(R.LARGE_N)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(family, k):
    """tokens at the largest count this K runs at, the codebook, the oracle's answer and (duplicate family) the index that must win; computed
    once and left unchanged"""
    n = N_MAX if k in R.LARGE_K else max(R.SMALL_N)
    lower = None
    if family == "duplicate":
        z, cb, lower = R.duplicate(n, k)
    else:
        z, cb = R.family(family, n, k)
    idx, zq = R.oracle(z, cb)
    for a in (z, cb, idx, zq):
        a.setflags(write=False)
    return z, cb, idx, zq, lower


def _check(family, n, k):
    z, cb, ridx, rzq, lower = _case(family, k)
    z, ridx, rzq = z[:n], ridx[:n], rzq[:n]
    zd, cbd = torch.from_numpy(np.array(z)).cuda(), torch.from_numpy(np.array(cb)).cuda()
    idx, zq = ops.vq_nearest(zd, cbd)
    idx2, zq2 = ops.vq_nearest(zd, cbd)
    idx3, none = ops.vq_nearest(zd, cbd, want_zq=False)
    torch.cuda.synchronize()
    tag = "%s:n%d:k%d" % (family, n, k)
    assert none is None and idx.dtype == torch.int64 and tuple(idx.shape) == (n,) and tuple(zq.shape) == (n, 3)
    got_idx, got_zq = idx.cpu().numpy(), zq.cpu().numpy()
    wrong = np.nonzero(got_idx != ridx)[0]
    assert wrong.size == 0, "%s: %d indices differ from the oracle, first token %d: %d, oracle %d" % (
        tag, wrong.size, wrong[0], got_idx[wrong[0]], ridx[wrong[0]])
    assert np.array_equal(_bits(got_zq), _bits(rzq)), tag + ": z_q differs from the oracle"
    assert np.array_equal(_bits(got_zq), _bits(cb[got_idx])), tag + ": z_q is not codebook[idx]"
    assert torch.equal(idx, idx2) and torch.equal(zq.view(torch.int32), zq2.view(torch.int32)), tag + ": two runs differ"
    assert torch.equal(idx, idx3), tag + ": want_zq=False changes the indices"
    ratio, _ = R.excess(zd, cbd, idx, device="cuda")
    within(float(ratio.max()), 1.0, "vq:" + tag)
    if lower is not None and lower.size:
        assert np.array_equal(got_idx, lower[:n]), tag + ": a duplicated row's upper copy won"
    if family == "special":
        assert got_idx[0] == 0 and np.array_equal(_bits(got_zq[0]), _bits(cb[0]))          # three NaN: no distance compares, index 0
        finite_rows = np.isfinite(cb).all(1)
        assert finite_rows.any() and bool(finite_rows[got_idx[np.isfinite(z).all(1)]].all()), tag + ": a NaN row was chosen"


@pytest.mark.parametrize("k", R.SMALL_K)
@pytest.mark.parametrize("n", R.SMALL_N)
def test_one_workgroup_every_code_count(n, k):
    """1 token; 127 / 128 / 129: one workgroup of 64 lanes x 2 tokens short of a token, full, and one token into the second.  16 code ranges:
    K = 7 and 3 leave most of them empty, K = 1 all but the last, K = 8193 / 16 385 leave a chunk of ONE code to the last range alone."""
    assert R.parts_for(n) == 16
    for family in R.FAMILIES:
        _check(family, n, k)


@pytest.mark.parametrize("k", R.LARGE_K)
@pytest.mark.parametrize("n", R.LARGE_N)
def test_every_launch_shape_both_sides_of_each_switch(n, k):
    assert R.parts_for(n) == (16 if n <= 32768 else 8 if n <= 65536 else 4)
    for family in R.FAMILIES:
        _check(family, n, k)


def test_outputs_are_written_inside_their_buffers():
    """idx and z_q inside filled buffers: n tokens written, the guard behind them kept, in each launch shape (the last workgroup ragged)"""
    k = 1000
    z, cb, ridx, rzq, _ = _case("midpoint0.7", k)
    cbd = torch.from_numpy(np.array(cb)).cuda()
    for n in (129, 32769, 65537 + 510):
        zd = torch.from_numpy(np.array(z[:n])).cuda()
        idx = torch.full((n + 64,), -7, dtype=torch.int64, device="cuda")
        zq = torch.full((n + 64, 3), -7.0, dtype=torch.float32, device="cuda")
        for want_zq in (True, False):
            idx.fill_(-7)
            zq.fill_(-7.0)
            st = _lib.lib().glare_vq_nearest_f32(ptr(zd), ptr(cbd), n, k, 3, ptr(idx), ptr(zq) if want_zq else None, stream_handle())
            torch.cuda.synchronize()
            assert st == 0
            assert np.array_equal(idx[:n].cpu().numpy(), ridx[:n]) and bool((idx[n:] == -7).all())
            if want_zq:
                assert np.array_equal(_bits(zq[:n].cpu().numpy()), _bits(rzq[:n])) and bool((zq[n:] == -7.0).all())
            else:
                assert bool((zq == -7.0).all())


def test_refusals_leave_the_outputs_alone():
    """test_gpu_vq.py::test_empty_and_errors through the C ABI, the outputs pre-filled: nothing may be launched"""
    n, k = 40, 8
    z = torch.randn(n, 3, device="cuda")
    cb = torch.randn(k, 3, device="cuda")
    idx = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    zq = torch.full((n, 3), -7.0, dtype=torch.float32, device="cuda")
    fn = _lib.lib().glare_vq_nearest_f32
    s = stream_handle()
    cases = [((ptr(z), ptr(cb), n, k, 4, ptr(idx), ptr(zq)), _lib.ERR_UNSUPPORTED),          # dim != 3
             ((ptr(z), ptr(cb), n, k, 2, ptr(idx), ptr(zq)), _lib.ERR_UNSUPPORTED),
             ((ptr(z), ptr(cb), n, 0, 3, ptr(idx), ptr(zq)), _lib.ERR_INVALID),
             ((ptr(z), ptr(cb), n, -1, 3, ptr(idx), ptr(zq)), _lib.ERR_INVALID),
             ((ptr(z), ptr(cb), -1, k, 3, ptr(idx), ptr(zq)), _lib.ERR_INVALID),
             ((None, ptr(cb), n, k, 3, ptr(idx), ptr(zq)), _lib.ERR_INVALID),
             ((ptr(z), None, n, k, 3, ptr(idx), ptr(zq)), _lib.ERR_INVALID),
             ((ptr(z), ptr(cb), n, k, 3, None, ptr(zq)), _lib.ERR_INVALID),
             ((ptr(z), ptr(cb), 0, k, 3, ptr(idx), ptr(zq)), 0),                             # an empty batch is no error and no launch
             ((None, None, 0, k, 3, None, None), 0)]
    for args, want in cases:
        assert fn(*args, s) == want, (args, want)
        torch.cuda.synchronize()
        assert bool((idx == -7).all()) and bool((zq == -7.0).all()), args
    e, none = ops.vq_nearest(torch.zeros(0, 3, device="cuda"), cb)
    assert e.numel() == 0
    with pytest.raises(Exception):
        ops.vq_nearest(torch.zeros(4, 4, device="cuda"), torch.zeros(8, 4, device="cuda"))
    assert fn(ptr(z), ptr(cb), n, k, 3, ptr(idx), ptr(zq), s) == 0                           # the same arguments without the fault
    torch.cuda.synchronize()
    assert bool((idx >= 0).all()) and torch.equal(zq, cb[idx])
