"""The semantics of glare_vq_restart_f32 (include/glare_hip.h) restated in numpy, shared by the restart tests.  Everything is an integer or a
bit copy: the tests compare bits, never within a tolerance."""
import numpy as np


def plan(window, threshold, n_tokens, offset):
    """-> (dead, t): the dead codes in ascending order (all D of them) and the source token of the first R = min(D, N)."""
    window = np.asarray(window, np.int64)
    dead = np.flatnonzero(window <= threshold).astype(np.int64)
    D, N = int(dead.size), int(n_tokens)
    R = min(D, N)
    if R == 0:
        return dead, np.zeros(0, np.int64)
    stride = N // R
    # Python integers: a true modulo for a negative offset, and no overflow
    t = np.array([(int(offset) + j * stride) % N for j in range(R)], np.int64)
    return dead, t


def restart(window, threshold, z, offset, codebook, exp_avg=None, exp_avg_sq=None):
    """-> dict(codebook, exp_avg, exp_avg_sq, window, n_dead, n_restarted, rows, tokens): the arrays after the call (copies; the moments
    None where none were given), and the rows actually written with the token each took."""
    z = np.asarray(z, np.float32)
    N = z.shape[0]
    dead, t = plan(window, threshold, N, offset)
    cb = np.array(codebook, np.float32, copy=True)
    m = None if exp_avg is None else np.array(exp_avg, np.float32, copy=True)
    v = None if exp_avg_sq is None else np.array(exp_avg_sq, np.float32, copy=True)
    ok = np.isfinite(z[t]).all(axis=1) if t.size else np.zeros(0, bool)
    rows, tokens = dead[:t.size][ok], t[ok]
    cb.view(np.uint32)[rows] = z.view(np.uint32)[tokens]          # a bit copy
    for mom in (m, v):
        if mom is not None:
            mom.view(np.uint32)[rows] = 0                          # +0.0
    return {"codebook": cb, "exp_avg": m, "exp_avg_sq": v, "window": np.zeros_like(np.asarray(window, np.int64)), "n_dead": int(dead.size),
            "n_restarted": int(rows.size), "rows": rows, "tokens": tokens}


def function_case(seed=0, n=512, k=8192):
    """The inputs of the function test: standard-normal latents and a codebook squeezed to 1e-4 x normal (every token then selects one of
    a few codes near the origin, and nearly the whole codebook is dead)."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, 3)).astype(np.float32)
    codebook = (1e-4 * rng.standard_normal((k, 3))).astype(np.float32)
    return z, codebook


FUNCTION_SEED = 0          # tests/test_vq_restart_host.py asserts on the CPU that the oracle search agrees for this seed
FUNCTION_OFFSET = 7919
