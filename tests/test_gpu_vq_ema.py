"""GPU: the EMA codebook kernels (csrc/vq_ema.hip) and the EMA restart (glare_vq_restart_ema_f32, csrc/vq_restart.hip) through the C ABI,
every buffer between guard bytes, against the fp64 restatement tests/vq_ema_oracle.py.

Counts are compared with array_equal.  Sums and the updated tensors go per element through fp64_bounds.assert_f32 with tolerances counted
from the kernels' source (U = 2^-24 per fp32 rounding):
  s_k            code k's tokens are added one by one within a segment (the first add, to +0, is exact) and the S segments' partial sums
                 one by one: segment s makes at most n_ks - 1 roundings relative to its own partial sum (<= its tokens' sum |z_i|), the
                 second level S - 1 relative to at most sum_{i in k} |z_i| -- together below (max_s n_ks + S) U sum_{i in k} |z_i|, the
                 longest chain times the magnitude; S = min(32, ceil(N / 512)) segments of ceil(N / S) tokens, from the header
  the update     tests/vq_ema_oracle.update_bound with kernel_model: three roundings per EMA (1 - d is exact at d = 0.99 and 0.6), n
                 summed in fp64 and rounded to fp32 once, one rounding for K * eps, four for smoothed, one for the row's division,
                 each times the magnitude of what is rounded, the errors of cluster_size and n carried into the row.  The update is
                 fed the kernel's own stats, so its inputs are exact fp32 numbers.
Where the bound is exactly 0 (a code with nothing to add to nothing) the result must be the restatement's exactly.
Shapes (N tokens, K codes): the smallest where each level can go wrong -- see SHAPES."""
import numpy as np
import pytest
import torch

import vq_ema_oracle as O
from fp64_bounds import assert_f32
from glare_amd import _lib, ops
from glare_amd._lib import stream_handle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 256                      # bytes on either side of every buffer
FILL = 0xA5

KMAX = _lib.constants()["GLARE_VQ_USAGE_MAX_CODES"]
# one code; a wave and a workgroup of codes, one below, at, one above; the 512-token tile and the one-segment limit at the trainer's K;
# 32 segments with a ragged last one; the sum of n at its widest (4096 workgroup sums)
SHAPES = [(1, 1), (5, 63), (5, 64), (5, 65), (300, 255), (300, 256), (300, 257), (511, 8192), (512, 8192), (513, 8192), (16385, 300), (64, KMAX)]
PATTERNS = ("uniform", "one_code", "out_of_range_mixed", "all_out_of_range")
ONCE_K = [1, 63, 64, 65, 255, 256, 257, 300, 8192]      # every code exactly once, N = K (N x K compares: K = 2^20 would take minutes)
DECAY, EPS = 0.99, 1e-5


class Guarded:
    """A device copy of a numpy array (or `nbytes` of FILL) between guard bytes (the pattern of tests/test_gpu_vq_restart.py)."""

    def __init__(self, array=None, nbytes=None):
        self.array = None if array is None else np.ascontiguousarray(array)
        self.n = self.array.nbytes if array is not None else nbytes
        self.buf = torch.full((2 * GUARD + self.n,), FILL, dtype=torch.uint8, device=DEV)
        if self.array is not None and self.n:
            self.buf[GUARD:GUARD + self.n] = torch.from_numpy(self.array.view(np.uint8).reshape(-1)).to(DEV)
        self.ptr = self.buf.data_ptr() + GUARD

    def read(self):
        """-> the bytes as the array's dtype and shape; asserts that the guards are as they were."""
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == FILL).all() and (b[GUARD + self.n:] == FILL).all(), "guard bytes were written"
        body = b[GUARD:GUARD + self.n]
        return body if self.array is None else body.view(self.array.dtype).reshape(self.array.shape)


def _segments(N):
    return min(32, max(1, -(-N // 512)))


def _abi_stats(idx, z, K):
    lib = _lib.main_lib()
    N = idx.shape[0]
    gi, gz = Guarded(idx), Guarded(z)
    gs = Guarded(np.full((K, 4), np.nan, np.float32))
    nws = lib.glare_vq_ema_workspace_bytes(N, K)
    assert nws == max(8 * ((K + 255) // 256 + 1), 16 * K * _segments(N) if _segments(N) > 1 else 0)
    ws = Guarded(nbytes=nws)
    _lib.check(lib.glare_vq_ema_stats_f32(gi.ptr, gz.ptr, N, K, 3, gs.ptr, ws.ptr, nws, stream_handle()), "glare_vq_ema_stats_f32")
    torch.cuda.synchronize()
    ws.read()
    assert gi.read().tobytes() == idx.tobytes() and gz.read().tobytes() == z.tobytes()
    return gs.read().copy()


def _abi_update(stats, cs, ea, E, decay, eps):
    lib = _lib.main_lib()
    K = cs.shape[0]
    gs, gc, ga, ge = Guarded(stats), Guarded(cs), Guarded(ea), Guarded(E)
    nws = lib.glare_vq_ema_workspace_bytes(1, K)
    assert nws == 8 * ((K + 255) // 256 + 1)
    ws = Guarded(nbytes=nws)
    _lib.check(lib.glare_vq_ema_update_f32(gs.ptr, K, 3, decay, eps, gc.ptr, ga.ptr, ge.ptr, ws.ptr, nws, stream_handle()),
               "glare_vq_ema_update_f32")
    torch.cuda.synchronize()
    ws.read()
    assert gs.read().tobytes() == stats.tobytes()
    return gc.read().copy(), ga.read().copy(), ge.read().copy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _assert_within(got, want, bound, tag):
    """per element |got - want| <= bound through assert_f32; where bound == 0, equality."""
    zero = bound == 0
    assert np.array_equal(got[zero].astype(np.float64), want[zero]), tag
    assert np.isfinite(want).all() and np.isfinite(got).all(), tag
    return assert_f32(_t(got), _t(want), _t(np.where(zero, 1.0, bound)), tag)


def _indices(pattern, N, K, rng):
    if pattern == "one_code":
        return np.full(N, K // 2, np.int64)                          # the longest chain: every token of every segment on one code
    if pattern == "all_out_of_range":
        return rng.choice(np.array([-1, K, 2 ** 40, -2 ** 40, K + 7], np.int64), N)
    idx = rng.integers(0, K, N).astype(np.int64)
    if pattern == "out_of_range_mixed":
        idx[rng.permutation(N)[:max(1, N // 3)]] = rng.choice(np.array([-1, K, 2 ** 40], np.int64), max(1, N // 3))
    return idx


def _longest_chain(idx, K):
    """per code: the most tokens it has within one segment, plus the segments"""
    N = idx.shape[0]
    S = _segments(N)
    seg_len = -(-N // S)
    most = np.zeros(K, np.int64)
    for a in range(0, N, seg_len):
        part = idx[a:a + seg_len]
        most = np.maximum(most, np.bincount(part[(part >= 0) & (part < K)], minlength=K))
    return most + S


def _check_case(idx, z, K, rng, tag, decay=DECAY, eps=EPS, zero_state=False):
    N = idx.shape[0]
    s, n_k, mag = O.stats(idx, z, K)
    stats = _abi_stats(idx, z, K)
    assert np.array_equal(stats[:, 3].astype(np.int64), n_k) and np.array_equal(stats[:, 3], n_k.astype(np.float32)), tag
    assert n_k.sum() == int(((idx >= 0) & (idx < K)).sum())
    assert not stats[:, :3].view(np.uint32)[n_k == 0].any(), tag    # nothing selected the code: +0.0
    r = _assert_within(stats[:, :3], s, _longest_chain(idx, K)[:, None] * O.U * mag, "stats")
    # the update, fed the kernel's own statistics
    if zero_state:
        cs0 = np.zeros(K, np.float32)
    else:
        cs0 = (np.abs(rng.standard_normal(K)) * max(1.0, N / K)).astype(np.float32)
        cs0[rng.random(K) < 0.5] = 0.0                              # codes that were never counted before
    ea0, E0 = (rng.standard_normal((K, 3)).astype(np.float32) for _ in range(2))
    got = _abi_update(stats, cs0, ea0, E0, decay, eps)
    s32, n32 = stats[:, :3].astype(np.float64), stats[:, 3].astype(np.int64)
    want = O.update(s32, n32, cs0, ea0, E0, decay, eps)
    bound = O.update_bound(O.kernel_model(decay, eps, K), s32, n32, cs0, ea0, decay, eps)
    if want[0].sum() == 0.0:                                         # n == 0: the rows keep their bits
        assert zero_state and not n_k.any()
        assert np.array_equal(got[2].view(np.uint32), E0.view(np.uint32)) and not got[0].any(), tag
        names = ("cluster_size", "embed_avg")
    else:
        names = ("cluster_size", "embed_avg", "codebook")
    ratios = [_assert_within(g, w, b, name) for name, g, w, b in zip(names, got, want, bound)]
    print(tag, "N", N, "K", K, "err / bound: stats %.3f" % r, " ".join("%s %.3f" % p for p in zip(names, ratios)))
    # determinism: a second run of both calls on fresh copies, identical bits
    stats2 = _abi_stats(idx, z, K)
    assert stats2.tobytes() == stats.tobytes(), tag
    again = _abi_update(stats2, cs0, ea0, E0, decay, eps)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), tag


@pytest.mark.parametrize("N,K", SHAPES, ids=["N%d-K%d" % s for s in SHAPES])
def test_stats_and_update_match_the_restatement(N, K):
    rng = np.random.default_rng(N * 11 + K)
    z = rng.standard_normal((N, 3)).astype(np.float32)
    for pattern in PATTERNS:
        _check_case(_indices(pattern, N, K, rng), z, K, rng, pattern, zero_state=pattern == "all_out_of_range")
    # a state that was never counted and indices that count now, and another decay (1 - 0.6 is exact in fp32 as well) and eps
    _check_case(_indices("uniform", N, K, rng), z, K, rng, "uniform_from_zero", zero_state=True)
    _check_case(_indices("uniform", N, K, rng), z, K, rng, "uniform_d0.6", decay=0.6, eps=1e-3)


@pytest.mark.parametrize("K", ONCE_K)
def test_every_code_exactly_once(K):
    rng = np.random.default_rng(K)
    idx = rng.permutation(K).astype(np.int64)
    z = rng.standard_normal((K, 3)).astype(np.float32)
    stats = _abi_stats(idx, z, K)
    assert (stats[:, 3] == 1.0).all()
    assert np.array_equal(stats[idx, :3].view(np.uint32), z.view(np.uint32))          # one term: the sum IS the token (0 + z, or z + 0 per segment)
    _check_case(idx, z, K, rng, "once")


def test_ops_follow_the_abi_and_refuse():
    N, K = 513, 300
    rng = np.random.default_rng(9)
    idx, z = rng.integers(0, K, N).astype(np.int64), rng.standard_normal((N, 3)).astype(np.float32)
    cs0, ea0, E0 = np.abs(rng.standard_normal(K)).astype(np.float32), *(rng.standard_normal((K, 3)).astype(np.float32) for _ in range(2))
    stats = ops.vq_ema_stats(_t(idx).to(DEV), _t(z).to(DEV), K)
    assert stats.dtype == torch.float32 and tuple(stats.shape) == (K, 4) and stats.is_cuda
    want = _abi_stats(idx, z, K)
    assert stats.cpu().numpy().tobytes() == want.tobytes()
    cs, ea, E = (_t(a).to(DEV) for a in (cs0, ea0, E0))
    assert ops.vq_ema_update(stats, cs, ea, E, DECAY, EPS) is None
    for got, ref in zip((cs, ea, E), _abi_update(want, cs0, ea0, E0, DECAY, EPS)):
        assert got.cpu().numpy().tobytes() == ref.tobytes()
    for decay, eps in ((0.0, EPS), (1.0, EPS), (DECAY, -1.0)):
        with pytest.raises(AssertionError):
            ops.vq_ema_update(stats, cs, ea, E, decay, eps)
    with pytest.raises(AssertionError):
        ops.vq_ema_update(stats[:-1], cs, ea, E, DECAY, EPS)
    with pytest.raises(AssertionError):
        ops.vq_ema_stats(_t(idx).to(DEV), _t(z[:-1]).to(DEV), K)
    with pytest.raises(_lib.GlareError) as e:
        ops.vq_ema_stats(torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, 3, device=DEV), KMAX + 1)
    assert e.value.status == _lib.ERR_UNSUPPORTED


def _abi_restart(ema, window, threshold, z, offset, codebook, ea, cs, seed):
    """glare_vq_restart_ema_f32 (ema) or glare_vq_restart_f32 without moments on fresh guarded copies -> dict of numpy results."""
    lib = _lib.main_lib()
    K, N = codebook.shape[0], z.shape[0]
    gw, gz, gc, ga, gs = Guarded(window), Guarded(z), Guarded(codebook), Guarded(ea), Guarded(cs)
    out = Guarded(np.full(2, -0x0123456789ABCDEF, np.int64))
    nws = lib.glare_vq_restart_workspace_bytes(K)
    ws = Guarded(nbytes=nws)
    if ema:
        _lib.check(lib.glare_vq_restart_ema_f32(gw.ptr, threshold, gz.ptr, N, K, 3, offset, seed, gc.ptr, ga.ptr, gs.ptr, out.ptr, out.ptr + 8,
                                                ws.ptr, nws, stream_handle()), "glare_vq_restart_ema_f32")
    else:
        _lib.check(lib.glare_vq_restart_f32(gw.ptr, threshold, gz.ptr, N, K, 3, offset, gc.ptr, None, None, out.ptr, out.ptr + 8, ws.ptr, nws,
                                            stream_handle()), "glare_vq_restart_f32")
    torch.cuda.synchronize()
    ws.read()
    assert gz.read().tobytes() == z.tobytes()
    n = out.read()
    return {"codebook": gc.read().copy(), "embed_avg": ga.read().copy(), "cluster_size": gs.read().copy(), "window": gw.read().copy(),
            "n_dead": int(n[0]), "n_restarted": int(n[1])}


@pytest.mark.parametrize("N,K", [(5, 65), (300, 257), (512, 8192)], ids=["N5-K65", "N300-K257", "N512-K8192"])
def test_restart_ema_is_the_restart_with_the_ema_state(N, K):
    rng = np.random.default_rng(N + 3 * K)
    z = rng.standard_normal((N, 3)).astype(np.float32)
    z[N // 2, 1] = np.inf                                            # a source token that re-seeds nothing, if the plan reaches it
    codebook, ea = (rng.standard_normal((K, 3)).astype(np.float32) for _ in range(2))
    cs = np.abs(rng.standard_normal(K)).astype(np.float32)
    for window, threshold, offset, seed in ((rng.integers(0, 3, K).astype(np.int64), 0, 3, 1.0), (np.zeros(K, np.int64), 0, -(3 * N + 7), 1.0),
                                            (rng.integers(0, 7, K).astype(np.int64), 3, 5 * N + 2, 2.5),
                                            (rng.integers(1, 9, K).astype(np.int64), 0, 0, 1.0)):
        plain = _abi_restart(False, window, threshold, z, offset, codebook, ea, cs, seed)
        got = _abi_restart(True, window, threshold, z, offset, codebook, ea, cs, seed)
        want = O.restart(window, threshold, z, offset, codebook, ea, cs, seed)
        tag = (N, K, threshold, offset, seed)
        print(tag, "dead", got["n_dead"], "restarted", got["n_restarted"])
        # for the same window, offset and threshold: the rows and the two counts of vq_restart, on bits; the plain call leaves the EMA state alone
        assert got["codebook"].tobytes() == plain["codebook"].tobytes() == want["codebook"].tobytes(), tag
        assert (got["n_dead"], got["n_restarted"]) == (plain["n_dead"], plain["n_restarted"]) == (want["n_dead"], want["n_restarted"]), tag
        assert plain["embed_avg"].tobytes() == ea.tobytes() and plain["cluster_size"].tobytes() == cs.tobytes(), tag
        assert not got["window"].any() and not plain["window"].any(), tag
        rows = want["rows"]
        assert got["embed_avg"].tobytes() == want["embed_avg"].tobytes() and got["cluster_size"].tobytes() == want["cluster_size"].tobytes(), tag
        assert np.array_equal(got["embed_avg"][rows].view(np.uint32), got["codebook"][rows].view(np.uint32)), tag
        assert (got["cluster_size"][rows] == np.float32(seed)).all(), tag
        live = np.ones(K, bool)
        live[rows] = False
        assert got["embed_avg"][live].tobytes() == ea[live].tobytes() and got["cluster_size"][live].tobytes() == cs[live].tobytes(), tag
        again = _abi_restart(True, window, threshold, z, offset, codebook, ea, cs, seed)
        assert all(np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes() for k in got), tag
    # through ops
    window = torch.zeros(K, dtype=torch.int64, device=DEV)
    cb_t, ea_t, cs_t = (_t(a).to(DEV) for a in (codebook, ea, cs))
    n_dead, n_restarted = ops.vq_restart_ema(window, _t(z).to(DEV), cb_t, ea_t, cs_t, 11)
    want = O.restart(np.zeros(K, np.int64), 0, z, 11, codebook, ea, cs, 1.0)
    assert int(n_dead) == K and int(n_restarted) == want["n_restarted"]
    assert cb_t.cpu().numpy().tobytes() == want["codebook"].tobytes() and ea_t.cpu().numpy().tobytes() == want["embed_avg"].tobytes()
    assert cs_t.cpu().numpy().tobytes() == want["cluster_size"].tobytes()
