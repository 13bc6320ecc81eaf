"""CPU: the EMA codebook's restatement (tests/vq_ema_oracle.py) against the reference's own EmbeddingEMA (tests/golden/vq_ema*.npz) and on
its own invariants, the typed C ABI of csrc/vq_ema.hip and of glare_vq_restart_ema_f32 with the refusals that return before anything is
launched, the ops' and the driver's refusals, and train.exchange_ema_stats on two gloo ranks."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import vq_ema_oracle as O
from glare_amd import _lib, fit, train

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(64, 512), (64, 2000), (300, 512), (300, 2000), (8192, 512), (8192, 2000)]


def _golden(K, N):
    g = np.load(os.path.join(GOLDEN, "vq_ema_large.npz" if (K, N) == (8192, 2000) else "vq_ema.npz"))
    tag = "K%d_N%d" % (K, N)
    return float(g["decay"]), float(g["eps"]), {k: g["%s_%s" % (k, tag)] for k in ("weight0", "idx", "z", "cluster_size", "embed_avg", "weight")}


@pytest.mark.parametrize("K,N", CASES, ids=["K%d-N%d" % c for c in CASES])
def test_restatement_matches_the_reference_module(K, N):
    """Three chained updates of the fp64 restatement against the fp32 tensors EmbeddingEMA left after each (quantize.py:345-358).  The bound
    is per element and derived, not measured: O.update_bound charges U = 2^-24 for every fp32 rounding of the reference's expressions
    (three per EMA, four for smoothed, one for the row's division), (n_k - 1) roundings for the n_k non-zero terms of the one-hot matmul
    `encodings.T @ z` (adding a zero is exact) relative to the sum of the |z| it adds, (K - 1) roundings for `cluster_size.sum()`, 2 U for
    num_tokens * eps, and the distance between the reference's alpha = f32(1 - 0.99) and the restatement's 1 - f32(0.99), 0.95e-6 relative;
    the errors of one update's state are carried into the next.  The counts are integers below 2^24: exact."""
    decay, eps, g = _golden(K, N)
    model = O.reference_model(decay, eps, K)
    assert 0.9e-6 < model.alpha_rel < 1.0e-6 and model.keps_rel == 2 * O.U
    cs, ea, E = np.zeros(K), g["weight0"].astype(np.float64), g["weight0"].astype(np.float64)
    e_cs, e_ea = np.zeros(K), np.zeros((K, 3))
    worst = 0.0
    for u in range(3):
        s, n_k, mag = O.stats(g["idx"][u], g["z"][u], K)
        assert n_k.sum() == N
        err_s = np.maximum(n_k - 1, 0)[:, None] * O.U * mag * O.FIRST_ORDER
        b_cs, b_ea, b_E = O.update_bound(model, s, n_k, cs, ea, decay, eps, err_s=err_s, err_cs=e_cs, err_ea=e_ea)
        cs, ea, E = O.update(s, n_k, cs, ea, E, decay, eps)
        for name, want, got, bound in (("cluster_size", cs, g["cluster_size"][u], b_cs), ("embed_avg", ea, g["embed_avg"][u], b_ea),
                                       ("weight", E, g["weight"][u], b_E)):
            err = np.abs(got.astype(np.float64) - want)
            zero = bound == 0
            assert (err[zero] == 0).all(), (name, u)
            ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
            rel = float((err / np.maximum(np.abs(want), 1e-300)).max())
            print("K %d N %d update %d %-12s max err / bound %.3f   max relative error %.3g" % (K, N, u + 1, name, ratio, rel))
            assert ratio < 1.0, (name, u, ratio)
            worst = max(worst, ratio)
        e_cs, e_ea = b_cs, b_ea
    dead = np.setdiff1d(np.arange(K), np.unique(g["idx"]))
    assert dead.size > 0 and np.abs(E[dead]).max() > 1e3            # the reference's dead codes are thrown far away (the issue's finding)
    assert worst > 0.01                                              # the bound is of the error's own order, not a formality


def test_restatement_invariants():
    rng = np.random.default_rng(5)
    for N, K in ((1, 1), (5, 64), (300, 257), (513, 8192), (4000, 300)):
        z = rng.standard_normal((N, 3)).astype(np.float32)
        idx = rng.integers(0, max(1, K // 2), N).astype(np.int64)               # the upper half of the codes is never selected
        bad = np.zeros(N, bool)
        if N >= 5:
            idx[1], idx[2], idx[4] = -1, K, 2 ** 40
            bad[[1, 2, 4]] = True
        s, n_k, mag = O.stats(idx, z, K)
        assert n_k.sum() == N - bad.sum() and (n_k >= 0).all()                   # sum n_k = N minus the tokens out of range
        assert np.allclose(s.sum(0), z[~bad].astype(np.float64).sum(0), atol=1e-9) and (mag >= np.abs(s) - 1e-12).all()
        cs0, ea0, E0 = np.abs(rng.standard_normal(K)), rng.standard_normal((K, 3)), rng.standard_normal((K, 3))
        cs, ea, E = O.update(s, n_k, cs0, ea0, E0, 0.99, 1e-5)
        d = O._f32(0.99)
        unused = n_k == 0
        assert np.array_equal(cs[unused], d * cs0[unused]) and np.array_equal(ea[unused], d * ea0[unused])      # n_k = 0: only decays
        n = cs.sum()
        assert np.allclose(E * ((cs + O._f32(1e-5)) / (n + K * O._f32(1e-5)) * n)[:, None], ea, rtol=1e-12)
        # n == 0: nothing was ever counted and nothing is now -- E stays, the state still decays
        none = np.full(N, K + 3, np.int64)
        s0, n0, _ = O.stats(none, z, K)
        assert not n0.any() and not s0.any()
        cs, ea, E = O.update(s0, n0, np.zeros(K), ea0, E0, 0.99, 1e-5)
        assert np.array_equal(E, E0) and not cs.any() and np.array_equal(ea, d * ea0)
        b = O.update_bound(O.kernel_model(0.99, 1e-5, K), s0, n0, np.zeros(K), ea0, 0.99, 1e-5)
        assert not b[2].any() and not b[0].any()
    # the restart under EMA: vq_restart_oracle's rows, embed_avg follows the codebook, cluster_size the seed
    K, N = 300, 40
    window = rng.integers(0, 3, K).astype(np.int64)
    z = rng.standard_normal((N, 3)).astype(np.float32)
    cb, ea = (rng.standard_normal((K, 3)).astype(np.float32) for _ in range(2))
    cs = np.abs(rng.standard_normal(K)).astype(np.float32)
    out = O.restart(window, 0, z, 7, cb, ea, cs, seed_size=1.0)
    rows = out["rows"]
    plain = O.R.restart(window, 0, z, 7, cb)
    assert np.array_equal(rows, plain["rows"]) and np.array_equal(out["codebook"].view(np.uint32), plain["codebook"].view(np.uint32))
    assert 0 < rows.size == out["n_restarted"] == min(out["n_dead"], N)
    assert np.array_equal(out["embed_avg"][rows].view(np.uint32), out["codebook"][rows].view(np.uint32)) and (out["cluster_size"][rows] == 1.0).all()
    live = np.ones(K, bool)
    live[rows] = False
    assert np.array_equal(out["embed_avg"][live], ea[live]) and np.array_equal(out["cluster_size"][live], cs[live])


def test_header_types_the_ema_entries_and_they_refuse_before_launching():
    c = ctypes
    sigs = _lib.signatures()
    assert sigs["glare_vq_ema_workspace_bytes"] == (c.c_size_t, [c.c_longlong, c.c_int])
    assert sigs["glare_vq_ema_stats_f32"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_longlong, c.c_int, c.c_int, c.c_void_p, c.c_void_p,
                                                        c.c_size_t, c.c_void_p])
    assert sigs["glare_vq_ema_update_f32"] == (c.c_int, [c.c_void_p, c.c_int, c.c_int, c.c_float, c.c_float] + [c.c_void_p] * 4
                                               + [c.c_size_t, c.c_void_p])
    assert sigs["glare_vq_restart_ema_f32"] == (c.c_int, [c.c_void_p, c.c_longlong, c.c_void_p, c.c_longlong, c.c_int, c.c_int, c.c_longlong,
                                                          c.c_float] + [c.c_void_p] * 6 + [c.c_size_t, c.c_void_p])
    kmax = _lib.constants()["GLARE_VQ_USAGE_MAX_CODES"]
    lib = _lib.lib()
    assert lib.glare_version() >= 128
    ws = lib.glare_vq_ema_workspace_bytes
    # one segment: the update's workgroup sums and n (fp64); more: the partial rows of 16 bytes per code and segment where they are larger
    assert ws(1, 1) == 16 and ws(512, 8192) == 8 * 33 and ws(513, 8192) == 2 * 8192 * 16 and ws(16385, 300) == 32 * 300 * 16
    assert ws(1 << 24, 300) == 32 * 300 * 16 and ws(64, kmax) == 8 * 4097
    assert ws(0, 8) == 0 and ws(8, 0) == 0 and ws(-1, 8) == 0 and ws((1 << 24) + 1, 8) == 0 and ws(8, kmax + 1) == 0
    buf = (c.c_longlong * 64)()                                   # host memory: every call below returns before it would be read
    p = c.addressof(buf)
    INV, UNS, WSP = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    f = lib.glare_vq_ema_stats_f32
    for i in (0, 1, 5, 6):                                        # idx, z, stats, workspace
        args = [p, p, 8, 8, 3, p, p, 1 << 20, None]
        args[i] = None
        assert f(*args) == INV, i
    for n, k, d in ((0, 8, 3), (-8, 8, 3), (8, 0, 3), (8, -8, 3), (8, 8, 0)):
        assert f(p, p, n, k, d, p, p, 1 << 20, None) == INV
    assert f(p, p, 8, 8, 3, p, p + 4, 1 << 20, None) == INV                        # a workspace that is not 8-byte aligned
    assert f(p, p, 8, 8, 4, p, p, 1 << 20, None) == UNS and f(p, p, 8, 8, 2, p, p, 1 << 20, None) == UNS
    assert f(p, p, (1 << 24) + 1, 8, 3, p, p, 1 << 40, None) == UNS               # the float count would no longer be exact
    assert f(p, p, 8, kmax + 1, 3, p, p, 1 << 40, None) == UNS
    assert f(p, p, 8, 8, 3, p, p, ws(8, 8) - 1, None) == WSP and f(p, p, 600, 8, 3, p, p, ws(600, 8) - 1, None) == WSP
    f = lib.glare_vq_ema_update_f32
    for i in (0, 5, 6, 7, 8):                                     # stats, cluster_size, embed_avg, codebook, workspace
        args = [p, 8, 3, 0.99, 1e-5, p, p, p, p, 1 << 20, None]
        args[i] = None
        assert f(*args) == INV, i
    for k, d in ((0, 3), (-8, 3), (8, 0)):
        assert f(p, k, d, 0.99, 1e-5, p, p, p, p, 1 << 20, None) == INV
    for decay, eps in ((0.0, 1e-5), (1.0, 1e-5), (-0.5, 1e-5), (1.5, 1e-5), (float("nan"), 1e-5), (0.99, -1e-5), (0.99, float("nan"))):
        assert f(p, 8, 3, decay, eps, p, p, p, p, 1 << 20, None) == INV, (decay, eps)
    assert f(p, 8, 3, 0.99, 1e-5, p, p, p, p + 4, 1 << 20, None) == INV
    assert f(p, 8, 4, 0.99, 1e-5, p, p, p, p, 1 << 20, None) == UNS
    assert f(p, kmax + 1, 3, 0.99, 1e-5, p, p, p, p, 1 << 40, None) == UNS
    assert f(p, 8, 3, 0.99, 1e-5, p, p, p, p, ws(1, 8) - 1, None) == WSP
    f = lib.glare_vq_restart_ema_f32
    rws = lib.glare_vq_restart_workspace_bytes
    for i in (0, 2, 8, 9, 10, 11, 12, 13):                        # window, z, codebook, embed_avg, cluster_size, n_dead, n_restarted, workspace
        args = [p, 0, p, 8, 8, 3, 0, 1.0, p, p, p, p, p, p, 1 << 20, None]
        args[i] = None
        assert f(*args) == INV, i
    for n, k, d in ((0, 8, 3), (-8, 8, 3), (8, 0, 3), (8, 8, 0)):
        assert f(p, 0, p, n, k, d, 0, 1.0, p, p, p, p, p, p, 1 << 20, None) == INV
    for seed in (-1.0, float("inf"), float("nan")):
        assert f(p, 0, p, 8, 8, 3, 0, seed, p, p, p, p, p, p, 1 << 20, None) == INV
    assert f(p, 0, p, 8, 8, 3, 0, 1.0, p, p, p, p, p, p + 4, 1 << 20, None) == INV
    assert f(p, 0, p, 8, 8, 4, 0, 1.0, p, p, p, p, p, p, 1 << 20, None) == UNS
    assert f(p, 0, p, 8, kmax + 1, 3, 0, 1.0, p, p, p, p, p, p, 1 << 40, None) == UNS
    assert f(p, 0, p, 8, 8, 3, 0, 1.0, p, p, p, p, p, p, rws(8) - 1, None) == WSP
    assert not any(buf)


def test_ops_and_trainer_surface_without_a_gpu():
    from glare_amd import ops

    K = 8
    with pytest.raises(NotImplementedError):
        ops.vq_ema_stats(torch.zeros(4, dtype=torch.int64), torch.zeros(4, 3), K)
    with pytest.raises(NotImplementedError):
        ops.vq_ema_update(torch.zeros(K, 4), torch.zeros(K), torch.zeros(K, 3), torch.zeros(K, 3), 0.99, 1e-5)
    with pytest.raises(NotImplementedError):
        ops.vq_restart_ema(torch.zeros(K, dtype=torch.int64), torch.zeros(4, 3), torch.zeros(K, 3), torch.zeros(K, 3), torch.zeros(K), 0)
    assert train.EMA_KEY == "codebook_ema"
    from glare_amd import modules as M

    q = M.VQModel().quantize
    assert q.loss_weights() == (q.beta, 1.0) and not q.ema_update                 # what train_nhwc derived from `legacy` before
    q.legacy = True
    assert q.loss_weights() == (1.0, q.beta)
    q.ema_update = True
    assert q.loss_weights() == (q.beta, 0.0)                                        # quantize.py:437, whatever `legacy` says
    with pytest.raises(AssertionError):
        train.Stage1Trainer(M.VQModel(), codebook_ema=1.0)
    with pytest.raises(AssertionError):
        train.Stage1Trainer(M.VQModel(), codebook_ema=0.0)


def test_codebook_ema_is_refused_for_stages_2_and_3_and_outside_its_range(capsys):
    for stage in ("stage2", "stage3"):
        with pytest.raises(ValueError) as e:
            fit.build_trainer(stage, fit.default_options(stage), "cpu", codebook_ema=0.99)
        assert str(e.value) == fit.CODEBOOK_EMA_REFUSAL
        with pytest.raises(ValueError) as e:
            fit.build_trainer(stage, fit.default_options(stage), "cpu", ema_eps=1e-5)
        assert str(e.value) == fit.CODEBOOK_EMA_REFUSAL
        with pytest.raises(SystemExit):
            fit.parse_args([stage, "--root", "x", "--out", "y", "--codebook-ema", "0.99"])
        assert "--codebook-ema / --ema-eps are stage1 options" in capsys.readouterr().err
    for bad in ("0", "1", "1.5", "-0.2", "nan"):
        with pytest.raises(SystemExit):
            fit.parse_args(["stage1", "--root", "x", "--out", "y", "--codebook-ema", bad])
        assert "a number in (0, 1)" in capsys.readouterr().err
        with pytest.raises(ValueError, match=r"a number in \(0, 1\)"):
            fit.build_trainer("stage1", fit.default_options("stage1"), "cpu", codebook_ema=float(bad))
    with pytest.raises(SystemExit):
        fit.parse_args(["stage1", "--root", "x", "--out", "y", "--ema-eps", "1e-5"])
    assert "--ema-eps needs --codebook-ema" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        fit.parse_args(["stage1", "--root", "x", "--out", "y", "--codebook-ema", "0.99", "--ema-eps", "-1"])
    args, _ = fit.parse_args(["stage1", "--root", "x", "--out", "y", "--codebook-ema", "0.99", "--ema-eps", "1e-6", "--codebook-restart", "100"])
    assert args.codebook_ema == 0.99 and args.ema_eps == 1e-6 and args.codebook_restart == 100
    args, _ = fit.parse_args(["stage1", "--root", "x", "--out", "y"])
    assert args.codebook_ema is None and args.ema_eps is None


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    stats = torch.arange(64, dtype=torch.float32).view(16, 4) * (rank + 1)
    out = train.exchange_ema_stats(stats, 5)
    refused = False
    try:
        train.exchange_ema_stats(stats.clone(), (1 << 23) + 1)            # world * N > 2^24: before any collective, on every rank
    except AssertionError:
        refused = True
    q.put((rank, out.clone(), out is stats, refused))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_exchange_ema_stats_on_two_gloo_ranks():
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
    for rank, stats, in_place, refused in got:
        assert torch.equal(stats, torch.arange(64, dtype=torch.float32).view(16, 4) * 3) and in_place and refused      # the statistics sum


def test_exchange_ema_stats_is_the_identity_without_a_process_group():
    stats = torch.arange(8, dtype=torch.float32).view(2, 4)
    out = train.exchange_ema_stats(stats, 1 << 30)
    assert out is stats and stats.flatten().tolist() == list(range(8))
