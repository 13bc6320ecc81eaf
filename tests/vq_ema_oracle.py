"""The semantics of glare_vq_ema_stats_f32 / glare_vq_ema_update_f32 / glare_vq_restart_ema_f32 (include/glare_hip.h) restated in fp64
numpy, with the first-order error analysis the EMA tests bound an fp32 evaluation by.  A plain module, shared by tests/test_vq_ema_host.py
(against the reference's own EmbeddingEMA, tests/golden/vq_ema.npz) and tests/test_gpu_vq_ema.py (against the kernels).

Scalar arguments are the C floats the ABI receives: d = f32(decay), eps = f32(eps), seed = f32(seed_size); 1 - d is then exact in fp64.

The error analysis (`update_bound`) walks the expressions of quantize.py:346-358 in the order they are evaluated and charges U = 2^-24
relative for every fp32 rounding, carrying the absolute error of each quantity forward to first order (the products of two errors are
below 2^-40 relative and are covered by the factor FIRST_ORDER).  What differs between the two fp32 evaluations it serves is a `Model`:
how far its 1 - d is from the restatement's, how many roundings its sum of n and its K * eps take."""
import collections
import math

import numpy as np

import vq_restart_oracle as R

U = 2.0 ** -24
FIRST_ORDER = 1.0 + 2.0 ** -10          # the second-order terms of the analysis: below 2^-40 relative, charged at 2^-10 of the bound


def _f32(v):
    """a Python number as the C `float` argument the ABI receives, back as a double (fp64_bounds._f32 without torch)"""
    return float(np.float32(v))


def stats(idx, z, n_codes):
    """-> (s fp64 [K,3], n_k int64 [K], mag fp64 [K,3]): the sum and the count of the tokens that select each code, and sum |z| of the
    same tokens (the magnitude the bound of a sum is stated in).  An index outside [0, K) selects nothing."""
    idx, z = np.asarray(idx, np.int64), np.asarray(z, np.float32).astype(np.float64)
    ok = (idx >= 0) & (idx < n_codes)
    k = idx[ok]
    n_k = np.bincount(k, minlength=n_codes).astype(np.int64)
    s, mag = np.zeros((n_codes, 3)), np.zeros((n_codes, 3))
    np.add.at(s, k, z[ok])
    np.add.at(mag, k, np.abs(z[ok]))
    return s, n_k, mag


def update(s, n_k, cluster_size, embed_avg, codebook, decay, eps):
    """-> (cluster_size, embed_avg, codebook) after one update, fp64 copies.  n == 0 exactly leaves the codebook as it was."""
    d, e = _f32(decay), _f32(eps)
    a = 1.0 - d
    K = len(n_k)
    cs = d * np.asarray(cluster_size, np.float64) + a * np.asarray(n_k, np.float64)
    ea = d * np.asarray(embed_avg, np.float64) + a * np.asarray(s, np.float64)
    n = math.fsum(cs.tolist())
    if n == 0.0:
        return cs, ea, np.array(codebook, np.float64, copy=True)
    smoothed = (cs + e) / (n + K * e) * n
    return cs, ea, ea / smoothed[:, None]


# alpha_rel: |its (1 - d) - the restatement's| / (1 - d);  n_sum_rel: the error of its sum of n relative to sum |cluster_size|;
# keps_rel: the error of its K * eps relative to K * eps
Model = collections.namedtuple("Model", "alpha_rel n_sum_rel keps_rel")


def reference_model(decay, eps, n_codes):
    """EmbeddingEMA on fp32 tensors: mul_(decay) takes f32(decay) -- the restatement's d -- but add_(alpha=1 - decay) takes f32(1 - decay) of
    the Python double, not 1 - f32(decay): the distance between the two is charged as it is (0.95e-6 relative at decay 0.99, the largest
    single term).  n = cluster_size.sum() is an fp32 sum of K terms in an order we do not know: (K - 1) roundings, each relative to at most
    the sum of the (non-negative) terms.  num_tokens * eps is f32 of the double product where the restatement has K * f32(eps): U for each."""
    d = _f32(decay)
    return Model(abs(_f32(1.0 - decay) - (1.0 - d)) / (1.0 - d), (n_codes - 1) * U, 2 * U)


def kernel_model(decay, eps, n_codes):
    """csrc/vq_ema.hip: 1 - d is an fp32 subtraction, exact for d >= 0.5 (Sterbenz) and one rounding below; n is summed in fp64 (K - 1
    roundings of 2^-53) and rounded to fp32 once; K * eps is one fp32 product of two exact operands."""
    return Model(0.0 if _f32(decay) >= 0.5 else U, U + (n_codes - 1) * 2.0 ** -53, U)


def update_bound(model, s, n_k, cluster_size, embed_avg, decay, eps, err_s=0.0, err_cs=0.0, err_ea=0.0):
    """-> (err_cs, err_ea, err_E): per-element bounds of |fp32 evaluation - update(...)| after one update, given bounds of the errors the
    evaluation's inputs already carry (err_s of its s_k; err_cs / err_ea of its state: 0 for inputs that are exact fp32 numbers).
    Roundings charged, each U relative to the magnitude of what is rounded:
      cluster_size  d * cs (1), a * n_k (1, n_k is exact), their sum (1)                                     [an FMA takes one fewer]
      embed_avg     d * ea (1), a * s_k (1), their sum (1)
      n             model.n_sum_rel * sum |cluster_size|, plus the errors of the terms
      smoothed      cs + eps (1), n + K eps (1, and model.keps_rel of K eps), the division (1), the product with n (1)
      E             the division (1)"""
    d, e = _f32(decay), _f32(eps)
    a = 1.0 - d
    K = len(n_k)
    cs0, ea0 = np.asarray(cluster_size, np.float64), np.asarray(embed_avg, np.float64)
    nk, s = np.asarray(n_k, np.float64), np.asarray(s, np.float64)
    cs, ea = d * cs0 + a * nk, d * ea0 + a * s
    e_cs = d * err_cs + U * np.abs(d * cs0) + (U + model.alpha_rel) * np.abs(a * nk) + U * np.abs(cs)
    e_ea = d * err_ea + U * np.abs(d * ea0) + a * err_s + (U + model.alpha_rel) * np.abs(a * s) + U * np.abs(ea)
    n = math.fsum(cs.tolist())
    if n == 0.0:
        return e_cs * FIRST_ORDER, e_ea * FIRST_ORDER, np.zeros_like(ea)
    e_n = float(np.sum(e_cs)) + model.n_sum_rel * float(np.sum(np.abs(cs)))
    den, num = n + K * e, cs + e
    e_den = e_n + model.keps_rel * K * e + U * abs(den)
    e_num = e_cs + U * np.abs(num)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_sm = e_num / np.abs(num) + e_den / abs(den) + U + e_n / abs(n) + U
        sm = num / den * n
        E = ea / sm[:, None]
        e_E = e_ea / np.abs(sm)[:, None] + np.abs(E) * (rel_sm + U)[:, None]
    return e_cs * FIRST_ORDER, e_ea * FIRST_ORDER, e_E * FIRST_ORDER


def restart(window, threshold, z, offset, codebook, embed_avg, cluster_size, seed_size=1.0):
    """-> dict(codebook, embed_avg, cluster_size, window, n_dead, n_restarted, rows, tokens): glare_vq_restart_ema_f32 on copies.  The rows,
    their tokens and the counts are vq_restart_oracle.restart's; a written row is also its embed_avg row, its cluster_size f32(seed_size)."""
    out = R.restart(window, threshold, z, offset, codebook)
    ea = np.array(embed_avg, np.float32, copy=True)
    cs = np.array(cluster_size, np.float32, copy=True)
    ea.view(np.uint32)[out["rows"]] = np.asarray(z, np.float32).view(np.uint32)[out["tokens"]]
    cs[out["rows"]] = np.float32(seed_size)
    out.update(embed_avg=ea, cluster_size=cs)
    del out["exp_avg"], out["exp_avg_sq"]
    return out
