"""GPU: the codebook-restart kernels (csrc/vq_restart.hip) through the C ABI and through glare_amd.ops, against tests/vq_restart_oracle.py.

Every output is an integer or a bit copy: each comparison is array_equal on the bits, there is no tolerance.  Shapes (N tokens, K codes):
the smallest at which each level of the dead codes' scan can go wrong -- one code; one below, at and one above a wave (64) and a workgroup
(256); the trainer's own 512 x 8192; several hundred workgroup totals with a ragged tail; and K = 2^20, the top-level scan at its widest.
Every buffer the call is handed lies between guard bytes."""
import numpy as np
import pytest
import torch

import vq_restart_oracle as R
from glare_amd import _lib, ops
from glare_amd._lib import stream_handle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KMAX = _lib.constants()["GLARE_VQ_USAGE_MAX_CODES"]
GUARD = 256                      # bytes on either side of every buffer
FILL = 0xA5
SHAPES = [(1, 1), (5, 63), (5, 64), (5, 65), (300, 255), (300, 256), (300, 257), (512, 8192), (4097, 70001), (64, KMAX)]
PATTERNS = ("none_dead", "all_dead", "every_other", "only_last", "only_first", "threshold_3", "offset_n", "offset_5n_2", "offset_negative",
            "no_moments", "nonfinite")


class Guarded:
    """A device copy of a numpy array (or `nbytes` of FILL) between guard bytes."""

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


def _abi_restart(window, threshold, z, offset, codebook, m, v):
    """One glare_vq_restart_f32 call on numpy arrays -> (codebook, m, v, window, n_dead, n_restarted) as numpy."""
    lib = _lib.main_lib()
    K, N = codebook.shape[0], z.shape[0]
    gw, gz, gc = Guarded(window), Guarded(z), Guarded(codebook)
    gm, gv = (None if a is None else Guarded(a) for a in (m, v))
    out = Guarded(np.full(2, -0x0123456789ABCDEF, np.int64))
    nws = lib.glare_vq_restart_workspace_bytes(K)
    assert nws == 32 + 12 * ((K + 255) // 256)          # the header, then three 32-bit cells per workgroup of 256 codes
    ws = Guarded(nbytes=nws)
    _lib.check(lib.glare_vq_restart_f32(gw.ptr, threshold, gz.ptr, N, K, 3, offset, gc.ptr, None if gm is None else gm.ptr,
                                        None if gv is None else gv.ptr, out.ptr, out.ptr + 8, ws.ptr, nws, stream_handle()),
               "glare_vq_restart_f32")
    torch.cuda.synchronize()
    ws.read()
    assert gz.read().tobytes() == np.ascontiguousarray(z).tobytes()                    # the latents are read only
    n = out.read()
    return gc.read(), None if gm is None else gm.read(), None if gv is None else gv.read(), gw.read(), int(n[0]), int(n[1])


def _bits(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint32)


def _case(pattern, N, K, rng):
    """-> (window, threshold, offset, with_moments) of a count pattern."""
    window = rng.integers(1, 50, K, dtype=np.int64)                      # nothing dead
    threshold, offset = 0, 3
    if pattern == "all_dead":
        window[:] = 0
    elif pattern in ("every_other", "offset_n", "offset_5n_2", "offset_negative", "no_moments", "nonfinite"):
        window[::2] = 0
        offset = {"offset_n": N, "offset_5n_2": 5 * N + 2, "offset_negative": -(3 * N + 7)}.get(pattern, 3)
    elif pattern == "only_last":
        window[K - 1] = 0
    elif pattern == "only_first":
        window[0] = 0
    elif pattern == "threshold_3":
        window, threshold = rng.integers(0, 7, K, dtype=np.int64), 3
    return window, threshold, offset, pattern != "no_moments"


@pytest.mark.parametrize("N,K", SHAPES, ids=["N%d-K%d" % s for s in SHAPES])
def test_restart_matches_the_restatement(N, K):
    rng = np.random.default_rng(N * 7 + K)
    z0 = rng.standard_normal((N, 3)).astype(np.float32)
    codebook = rng.standard_normal((K, 3)).astype(np.float32)
    m0 = rng.standard_normal((K, 3)).astype(np.float32)
    v0 = np.abs(rng.standard_normal((K, 3))).astype(np.float32)
    for pattern in PATTERNS:
        window, threshold, offset, with_moments = _case(pattern, N, K, rng)
        m, v = (m0, v0) if with_moments else (None, None)
        z, planted = z0, 0
        dead, t = R.plan(window, threshold, N, offset)
        assert len(set(t.tolist())) == t.size == min(dead.size, N)
        if pattern == "nonfinite":                                  # inf, -inf and NaN in the first, the middle and the last source token
            z = z0.copy()
            for j, (comp, bad) in zip(sorted({0, t.size // 2, t.size - 1}), ((0, np.inf), (2, np.nan), (1, -np.inf))):
                z[t[j], comp] = bad
                planted += 1
        want = R.restart(window, threshold, z, offset, codebook, m, v)
        got = _abi_restart(window, threshold, z, offset, codebook, m, v)
        cb, gm, gv, gw, n_dead, n_restarted = got
        tag = (pattern, N, K)
        print(tag, "dead", n_dead, "restarted", n_restarted)
        assert n_dead == want["n_dead"] == dead.size and n_restarted == want["n_restarted"] == t.size - planted, tag
        assert np.array_equal(_bits(cb), _bits(want["codebook"])), tag
        assert not gw.any(), tag                                        # the window is zero afterwards, whatever it held
        rows = want["rows"]
        assert np.array_equal(_bits(cb[rows]), _bits(z[want["tokens"]])), tag
        live = np.ones(K, bool)
        live[rows] = False
        assert np.array_equal(_bits(cb[live]), _bits(codebook[live])), tag
        if with_moments:
            assert np.array_equal(_bits(gm), _bits(want["exp_avg"])) and np.array_equal(_bits(gv), _bits(want["exp_avg_sq"])), tag
            assert not _bits(gm[rows]).any() and not _bits(gv[rows]).any(), tag          # +0.0: no sign bit
            assert np.array_equal(_bits(gm[live]), _bits(m0[live])) and np.array_equal(_bits(gv[live]), _bits(v0[live])), tag
        else:
            assert gm is None and gv is None
        if pattern == "none_dead":
            assert n_dead == n_restarted == 0 and rows.size == 0
        if pattern == "all_dead":
            assert n_dead == K and n_restarted == min(K, N) and np.array_equal(rows, np.arange(min(K, N))), tag
            assert len(set(want["tokens"].tolist())) == min(K, N)     # D > N: the first N codes, from N distinct tokens
        if pattern == "only_last":
            assert rows.tolist() == [K - 1]
        if pattern == "only_first":
            assert rows.tolist() == [0]
        if pattern == "nonfinite":
            assert planted >= 1 and np.isfinite(cb).all(), tag
            assert not np.isfinite(z[t]).all()
        if pattern == "threshold_3":                                     # determinism: a second launch on fresh copies, identical bits
            again = _abi_restart(window, threshold, z, offset, codebook, m, v)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], again[:4])) and got[4:] == again[4:], tag


def test_reseeded_codes_are_selected_by_their_tokens():
    """(N, K) = (512, 8192), standard-normal latents, a codebook squeezed to 1e-4 x normal, the window from a real vq_nearest + vq_usage of
    those latents: after the restart every re-seeded token finds its own code (tests/test_vq_restart_host.py asserts the same of the CPU
    oracle's search for this seed: the expanded distance does not let a neighbour win here)."""
    z_np, cb_np = R.function_case(R.FUNCTION_SEED)
    z, codebook = torch.from_numpy(z_np).to(DEV), torch.from_numpy(cb_np).to(DEV)
    K = codebook.shape[0]
    idx, _ = ops.vq_nearest(z, codebook)
    window = torch.zeros(K, dtype=torch.int64, device=DEV)
    _, _, total = ops.vq_usage(idx, K, total=window)
    assert total is window
    win_np = window.cpu().numpy()
    assert np.array_equal(win_np, np.bincount(idx.cpu().numpy(), minlength=K))
    want = R.restart(win_np, 0, z_np, R.FUNCTION_OFFSET, cb_np, np.ones_like(cb_np), np.ones_like(cb_np))
    m, v = torch.ones_like(codebook), torch.ones_like(codebook)
    n_dead, n_restarted = ops.vq_restart(window, z, codebook, R.FUNCTION_OFFSET, exp_avg=m, exp_avg_sq=v)
    assert n_dead.is_cuda and n_dead.dtype == n_restarted.dtype == torch.int64 and n_dead.dim() == n_restarted.dim() == 0
    assert int(n_dead) == want["n_dead"] > 512 and int(n_restarted) == want["n_restarted"] == 512
    assert np.array_equal(_bits(codebook.cpu().numpy()), _bits(want["codebook"])) and not bool(window.any())
    assert np.array_equal(_bits(m.cpu().numpy()), _bits(want["exp_avg"])) and torch.equal(m, v)
    idx2, _ = ops.vq_nearest(z, codebook)
    assert np.array_equal(idx2.cpu().numpy()[want["tokens"]], want["rows"])
    # without moments, and with a threshold
    n2 = ops.vq_restart(torch.full((K,), 2, dtype=torch.int64, device=DEV), z, codebook, -1, threshold=2)
    assert int(n2[0]) == K and int(n2[1]) == 512
    with pytest.raises(AssertionError):
        ops.vq_restart(window, z, codebook, 0, exp_avg=m)                 # one moment without the other


def test_bad_arguments_return_their_status_and_write_nothing():
    lib = _lib.main_lib()
    K, N = 300, 40
    rng = np.random.default_rng(1)
    window, z = Guarded(np.zeros(K, np.int64) + 0), Guarded(rng.standard_normal((N, 3)).astype(np.float32))
    window.buf[GUARD:GUARD + 8 * K] = FILL                                # a sentinel the kernels would have zeroed
    cb, m, v = (Guarded(nbytes=12 * K) for _ in range(3))
    out = Guarded(nbytes=16)
    nws = lib.glare_vq_restart_workspace_bytes(K)
    ws = Guarded(nbytes=nws)
    assert nws > 0 and lib.glare_vq_restart_workspace_bytes(0) == 0 and lib.glare_vq_restart_workspace_bytes(KMAX + 1) == 0
    assert lib.glare_vq_restart_workspace_bytes(KMAX) == 32 + 12 * (KMAX // 256)
    f, s = lib.glare_vq_restart_f32, stream_handle()
    W, Z, C, M, V, D, Rr, S = window.ptr, z.ptr, cb.ptr, m.ptr, v.ptr, out.ptr, out.ptr + 8, ws.ptr
    INV, UNS, WSP = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    assert f(None, 0, Z, N, K, 3, 0, C, M, V, D, Rr, S, nws, s) == INV
    assert f(W, 0, None, N, K, 3, 0, C, M, V, D, Rr, S, nws, s) == INV
    assert f(W, 0, Z, N, K, 3, 0, None, M, V, D, Rr, S, nws, s) == INV
    assert f(W, 0, Z, N, K, 3, 0, C, M, V, None, Rr, S, nws, s) == INV
    assert f(W, 0, Z, N, K, 3, 0, C, M, V, D, None, S, nws, s) == INV
    assert f(W, 0, Z, N, K, 3, 0, C, M, V, D, Rr, None, nws, s) == INV
    assert f(W, 0, Z, N, K, 3, 0, C, None, V, D, Rr, S, nws, s) == INV        # exactly one moment
    assert f(W, 0, Z, N, K, 3, 0, C, M, None, D, Rr, S, nws, s) == INV
    assert f(W, 0, Z, 0, K, 3, 0, C, M, V, D, Rr, S, nws, s) == INV
    assert f(W, 0, Z, -5, K, 3, 0, C, M, V, D, Rr, S, nws, s) == INV
    assert f(W, 0, Z, N, 0, 3, 0, C, M, V, D, Rr, S, nws, s) == INV
    assert f(W, 0, Z, N, K, 0, 0, C, M, V, D, Rr, S, nws, s) == INV
    assert f(W, 0, Z, N, K, 3, 0, C, M, V, D, Rr, S + 4, nws, s) == INV       # a workspace that is not 8-byte aligned
    assert f(W, 0, Z, N, K, 4, 0, C, M, V, D, Rr, S, nws, s) == UNS
    assert f(W, 0, Z, N, K, 2, 0, C, M, V, D, Rr, S, nws, s) == UNS
    assert f(W, 0, Z, N, KMAX + 1, 3, 0, C, M, V, D, Rr, S, 1 << 40, s) == UNS
    assert f(W, 0, Z, N, K, 3, 0, C, M, V, D, Rr, S, nws - 1, s) == WSP
    assert f(W, 0, Z, N, K, 3, 0, C, M, V, D, Rr, S, 0, s) == WSP
    torch.cuda.synchronize()
    for g in (window, cb, m, v, out, ws):
        assert bool((g.buf == FILL).all())
    with pytest.raises(_lib.GlareError) as e:
        ops.vq_restart(torch.zeros(KMAX + 1, dtype=torch.int64, device=DEV), torch.zeros(4, 3, device=DEV), torch.zeros(KMAX + 1, 3, device=DEV), 0)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        ops.vq_restart(torch.zeros(4, dtype=torch.int64), torch.zeros(4, 3), torch.zeros(4, 3), 0)
