"""The restatement every codebook-usage test is held to: np.bincount for the counts, and the reference's perplexity
(code/models/modules/quantize.py:83-85: e_mean = mean(one_hot(idx), 0); perplexity = exp(-sum(e_mean * log(e_mean + 1e-10)))) in float64
from those counts.  tests/test_usage_host.py pins it against the reference's own VectorQuantizer.forward."""
import math

import numpy as np

# the five seeded cases (K codes, N = h * w tokens of a [1, 3, h, w] latent) the restatement is pinned on
CASES = ((64, 4, 6), (8192, 12, 16), (8192, 100, 150), (37, 7, 15), (8192, 32, 64))


def counts(idx, n_codes, groups=1):
    """idx: integers, `groups` equal runs -> (int64 [groups, n_codes] counts, int64 [groups] indices outside [0, n_codes))."""
    idx = np.asarray(idx).astype(np.int64).reshape(groups, -1)
    out = np.zeros((groups, n_codes), np.int64)
    oor = np.zeros(groups, np.int64)
    for g in range(groups):
        ok = (idx[g] >= 0) & (idx[g] < n_codes)
        out[g] = np.bincount(idx[g][ok], minlength=n_codes)
        oor[g] = int((~ok).sum())
    return out, oor


def stats(row):
    """One int64 [K] histogram -> {"tokens", "active", "entropy", "perplexity", "abs_terms"}; abs_terms = sum_k |p_k log(p_k + 1e-10)|, what
    a bound on the summation error scales with.  A row without tokens: the sum is empty, perplexity 1."""
    row = np.asarray(row, dtype=np.int64)
    n = int(row.sum())
    if n == 0:
        return {"tokens": 0, "active": 0, "entropy": 0.0, "perplexity": 1.0, "abs_terms": 0.0}
    p = row.astype(np.float64) / np.float64(n)
    terms = p * np.log(p + 1e-10)
    h = -math.fsum(terms.tolist())
    return {"tokens": n, "active": int((row > 0).sum()), "entropy": h, "perplexity": math.exp(h), "abs_terms": math.fsum(np.abs(terms).tolist())}


def perplexity_bound(n_codes, abs_terms):
    """Relative bound of an fp64 evaluation of the expression above from exact counts, any summation order, log and exp within 1 ulp:
    (K + 8) * 2^-53 * (1 + sum |terms|)."""
    return (n_codes + 8) * 2.0 ** -53 * (1.0 + abs_terms)


def reference_case(case, seed):
    """(z [1, 3, h, w] fp32, codebook [K, 3] fp32) of a seeded case: normal latents over a normal codebook, so that many codes are in use."""
    import torch

    K, h, w = case
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 3, h, w, generator=g), torch.randn(K, 3, generator=g)
