"""CPU: the restart's restatement (tests/vq_restart_oracle.py) on its own invariants, the CPU oracle's agreement on the function test's
inputs, the typed C ABI of csrc/vq_restart.hip and its refusals (they return before anything is launched), the driver's refusals, and
train.exchange_restart_inputs on two gloo ranks."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import vq_restart_oracle as R
from glare_amd import _lib, fit, train


def test_restatement_invariants():
    rng = np.random.default_rng(0)
    for N, K, thr in ((1, 1, 0), (5, 64, 0), (300, 257, 3), (512, 8192, 0), (4097, 700, 2), (64, 5000, 6)):
        for offset in (0, 3, N, 5 * N + 2, -1, -(3 * N + 7)):
            window = rng.integers(0, 7, K, dtype=np.int64)
            z = rng.standard_normal((N, 3)).astype(np.float32)
            cb, m, v = (rng.standard_normal((K, 3)).astype(np.float32) for _ in range(3))
            dead, t = R.plan(window, thr, N, offset)
            D = int((window <= thr).sum())
            assert dead.size == D and np.array_equal(dead, np.sort(dead)) and t.size == min(D, N)                # R = min(D, N)
            assert len(set(t.tolist())) == t.size and (t >= 0).all() and (t < N).all()                            # the t_j are distinct
            if t.size:
                assert t[0] == offset % N
            out = R.restart(window, thr, z, offset, cb, m, v)
            assert out["n_dead"] == D and out["n_restarted"] == t.size and not out["window"].any()
            rows = out["rows"]
            assert np.array_equal(rows, dead[:t.size]) and np.array_equal(out["codebook"][rows], z[t])
            live = np.ones(K, bool)
            live[rows] = False
            for after, before in ((out["codebook"], cb), (out["exp_avg"], m), (out["exp_avg_sq"], v)):          # live rows are untouched
                assert np.array_equal(after[live].view(np.uint32), before[live].view(np.uint32))
            assert not out["exp_avg"][rows].view(np.uint32).any() and not out["exp_avg_sq"][rows].view(np.uint32).any()
    # a source token with an inf / NaN re-seeds nothing and is not counted
    window, z = np.zeros(4, np.int64), np.arange(12, dtype=np.float32).reshape(4, 3)
    z[1, 2], z[3, 0] = np.nan, -np.inf
    cb = np.full((4, 3), 7, np.float32)
    out = R.restart(window, 0, z, 0, cb)
    assert out["n_dead"] == 4 and out["n_restarted"] == 2 and out["rows"].tolist() == [0, 2] and out["exp_avg"] is None
    assert np.array_equal(out["codebook"], np.array([z[0], cb[1], z[2], cb[3]]))


def test_cpu_oracle_search_finds_every_reseeded_code():
    """The function test of tests/test_gpu_vq_restart.py asks that after the restart token t_j selects code d_j.  The search uses the
    expanded distance, so a neighbour could in principle win by rounding: for the seed the test uses, the CPU oracle says it does not."""
    from oracle import c_ref

    z, cb = R.function_case(R.FUNCTION_SEED)
    idx, _ = c_ref.vq_nearest(z, cb)
    window = np.bincount(idx, minlength=cb.shape[0]).astype(np.int64)
    out = R.restart(window, 0, z, R.FUNCTION_OFFSET, cb)
    assert out["n_dead"] > 512 and out["n_restarted"] == 512 and len(set(out["tokens"].tolist())) == 512
    idx2, _ = c_ref.vq_nearest(z, out["codebook"])
    assert np.array_equal(idx2[out["tokens"]], out["rows"])


def test_header_types_the_restart_entries_and_they_refuse_before_launching():
    c = ctypes
    sigs = _lib.signatures()
    assert sigs["glare_vq_restart_workspace_bytes"] == (c.c_size_t, [c.c_int])
    assert sigs["glare_vq_restart_f32"] == (c.c_int, [c.c_void_p, c.c_longlong, c.c_void_p, c.c_longlong, c.c_int, c.c_int, c.c_longlong]
                                            + [c.c_void_p] * 6 + [c.c_size_t, c.c_void_p])
    kmax = _lib.constants()["GLARE_VQ_USAGE_MAX_CODES"]
    lib = _lib.lib()
    assert lib.glare_version() >= 127
    ws = lib.glare_vq_restart_workspace_bytes
    assert ws(1) == 32 + 12 and ws(256) == 32 + 12 and ws(257) == 32 + 24 and ws(kmax) == 32 + 12 * 4096
    assert ws(0) == 0 and ws(-3) == 0 and ws(kmax + 1) == 0
    buf = (c.c_longlong * 64)()                                   # host memory: every call below returns before it would be read
    p = c.addressof(buf)
    f = lib.glare_vq_restart_f32
    for i in (0, 2, 7, 10, 11, 12):                               # window, z, codebook, n_dead, n_restarted, workspace
        args = [p, 0, p, 8, 8, 3, 0, p, p, p, p, p, p, 1 << 20, None]
        args[i] = None
        assert f(*args) == _lib.ERR_INVALID, i
    assert f(p, 0, p, 8, 8, 3, 0, p, None, p, p, p, p, 1 << 20, None) == _lib.ERR_INVALID         # exactly one moment pointer
    assert f(p, 0, p, 8, 8, 3, 0, p, p, None, p, p, p, 1 << 20, None) == _lib.ERR_INVALID
    for n, k, d in ((0, 8, 3), (-8, 8, 3), (8, 0, 3), (8, -8, 3), (8, 8, 0)):
        assert f(p, 0, p, n, k, d, 0, p, p, p, p, p, p, 1 << 20, None) == _lib.ERR_INVALID
    assert f(p, 0, p, 8, 8, 3, 0, p, p, p, p, p, p + 4, 1 << 20, None) == _lib.ERR_INVALID
    assert f(p, 0, p, 8, 8, 4, 0, p, p, p, p, p, p, 1 << 20, None) == _lib.ERR_UNSUPPORTED
    assert f(p, 0, p, 8, kmax + 1, 3, 0, p, p, p, p, p, p, 1 << 40, None) == _lib.ERR_UNSUPPORTED
    assert f(p, 0, p, 8, 8, 3, 0, p, None, None, p, p, p, ws(8) - 1, None) == _lib.ERR_WORKSPACE
    assert not any(buf)


def test_ops_and_trainer_surface_without_a_gpu():
    from glare_amd import ops

    with pytest.raises(NotImplementedError):
        ops.vq_restart(torch.zeros(8, dtype=torch.int64), torch.zeros(4, 3), torch.zeros(8, 3), 0)
    assert train.RESTART_TERMS == ("codebook_restarted",) and train.RESTART_KEY == "codebook_restart"


def test_codebook_restart_is_refused_for_stages_2_and_3(capsys):
    for stage in ("stage2", "stage3"):
        with pytest.raises(ValueError) as e:
            fit.build_trainer(stage, fit.default_options(stage), "cpu", codebook_restart=10)
        assert str(e.value) == fit.CODEBOOK_RESTART_REFUSAL
        with pytest.raises(ValueError) as e:
            fit.build_trainer(stage, fit.default_options(stage), "cpu", restart_threshold=1)
        assert str(e.value) == fit.CODEBOOK_RESTART_REFUSAL
        with pytest.raises(SystemExit):
            fit.parse_args([stage, "--root", "x", "--out", "y", "--codebook-restart", "10"])
        assert "--codebook-restart / --restart-threshold are stage1 options" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        fit.parse_args(["stage1", "--root", "x", "--out", "y", "--restart-threshold", "2"])
    assert "--restart-threshold needs --codebook-restart" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        fit.parse_args(["stage1", "--root", "x", "--out", "y", "--codebook-restart", "-1"])
    args, _ = fit.parse_args(["stage1", "--root", "x", "--out", "y", "--codebook-restart", "10", "--restart-threshold", "2"])
    assert args.codebook_restart == 10 and args.restart_threshold == 2
    args, _ = fit.parse_args(["stage1", "--root", "x", "--out", "y"])
    assert args.codebook_restart == 0 and args.restart_threshold is None


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    window = torch.arange(16, dtype=torch.int64) * (rank + 1)
    z = torch.full((5, 3), float(rank + 1))
    w2, z2 = train.exchange_restart_inputs(window, z)
    q.put((rank, w2.clone(), z2.clone(), w2 is window))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_exchange_restart_inputs_on_two_gloo_ranks():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=120) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, window, z, in_place in got:
        assert torch.equal(window, torch.arange(16, dtype=torch.int64) * 3) and in_place            # the windows sum
        assert torch.equal(z, torch.full((5, 3), 1.0))                                                  # both end with rank 0's latents


def test_exchange_restart_inputs_is_the_identity_without_a_process_group():
    window, z = torch.arange(4, dtype=torch.int64), torch.ones(2, 3)
    w2, z2 = train.exchange_restart_inputs(window, z)
    assert w2 is window and z2 is z and window.tolist() == [0, 1, 2, 3]
