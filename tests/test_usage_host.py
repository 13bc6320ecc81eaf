"""CPU: the codebook-usage restatement (tests/usage_fp64.py) against the reference's own VectorQuantizer.forward
(code/models/modules/quantize.py:83-85) where the reference is present, and against the committed fixture everywhere; the typed C ABI
of csrc/vq_usage.hip and its refusals, which return before anything is launched."""
import ctypes
import os

import numpy as np
import pytest

import usage_fp64 as U
from glare_amd import _lib
from oracle import refimport

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vq_usage.npz")
# The reference holds e_mean and the sum in fp32: (log2 K + 4) * 2^-24 * ln K at K = 8192 is 9.1e-6, rounded up.
REL = 1e-5


def _check(idx, K, ref_perplexity, ref_counts):
    counts, oor = U.counts(idx, K)
    assert oor.tolist() == [0] and np.array_equal(counts[0], ref_counts)
    s = U.stats(counts[0])
    assert s["tokens"] == idx.size and s["active"] == int((ref_counts > 0).sum()) and s["active"] >= 17         # not a degenerate case
    rel = abs(s["perplexity"] - float(ref_perplexity)) / float(ref_perplexity)
    print("K %d N %d active %d perplexity %.9g reference %.9g rel %.3g" % (K, idx.size, s["active"], s["perplexity"], float(ref_perplexity), rel))
    assert rel <= REL
    return s


@pytest.mark.skipif(not refimport.available(), reason="the reference tree is not present")
@pytest.mark.parametrize("i", range(len(U.CASES)))
def test_restatement_matches_the_reference_vector_quantizer(i):
    import sys

    sys.path.insert(0, os.path.dirname(GOLDEN))
    try:
        import make_vq_usage_golden as G
    finally:
        sys.path.pop(0)
    idx, perplexity, counts = G.run_reference(U.CASES[i], G.SEED0 + i)
    assert idx.size == U.CASES[i][1] * U.CASES[i][2]
    _check(idx, U.CASES[i][0], perplexity, counts)
    g = np.load(GOLDEN)                                        # and the fixture is what the reference computes today
    assert np.array_equal(g["idx_%d" % i], idx) and np.array_equal(g["counts_%d" % i], counts)
    assert abs(float(g["perplexity_%d" % i]) - float(perplexity)) <= REL * float(perplexity)


def test_restatement_matches_the_fixture():
    g = np.load(GOLDEN)
    assert int(g["n_cases"]) == len(U.CASES)
    for i, (K, h, w) in enumerate(U.CASES):
        assert int(g["K_%d" % i]) == K and g["idx_%d" % i].size == h * w
        _check(g["idx_%d" % i].astype(np.int64), K, g["perplexity_%d" % i], g["counts_%d" % i])


def test_restatement_edges():
    c, oor = U.counts([0, 5, -1, 5, 6, 2 ** 40, 3, 5], 6, groups=2)
    assert c.tolist() == [[1, 0, 0, 0, 0, 2], [0, 0, 0, 1, 0, 1]] and oor.tolist() == [1, 2]
    assert U.stats(np.zeros(7, np.int64)) == {"tokens": 0, "active": 0, "entropy": 0.0, "perplexity": 1.0, "abs_terms": 0.0}
    one = U.stats([0, 9, 0])
    assert one["active"] == 1 and one["perplexity"] == pytest.approx(1.0, abs=1e-9)        # exp(-log(1 + 1e-10))
    flat = U.stats(np.full(37, 3))
    assert flat["active"] == 37 and flat["perplexity"] == pytest.approx(37.0, rel=1e-8)
    assert U.perplexity_bound(8192, 9.0) == 8200 * 2.0 ** -53 * 10


def test_header_types_the_usage_entries_and_they_refuse_before_launching():
    c = ctypes
    sigs = _lib.signatures()
    assert sigs["glare_vq_usage_workspace_bytes"] == (c.c_size_t, [c.c_int, c.c_longlong, c.c_int])
    assert sigs["glare_vq_usage_i64"] == (c.c_int, [c.c_void_p, c.c_int, c.c_longlong, c.c_int] + [c.c_void_p] * 4 + [c.c_size_t, c.c_void_p])
    assert sigs["glare_vq_usage_stats"] == (c.c_int, [c.c_void_p, c.c_int, c.c_int] + [c.c_void_p] * 5)
    K = _lib.constants()
    tier, span, kmax = K["GLARE_VQ_USAGE_TIER"], K["GLARE_VQ_USAGE_SPAN"], K["GLARE_VQ_USAGE_MAX_CODES"]
    lib = _lib.lib()
    assert lib.glare_version() >= 126
    ws = lib.glare_vq_usage_workspace_bytes
    assert ws(1, 1, tier) == (tier + 1) * 4 and ws(3, span, 37) == 3 * 38 * 4 and ws(3, span + 1, 37) == 3 * 2 * 38 * 4
    assert ws(1, 10 ** 12, 5) == 64 * 6 * 4                                               # 64 spans at most
    assert ws(0, 5, 5) == 0 and ws(1, 0, 5) == 0 and ws(1, 5, 0) == 0 and ws(1, 5, kmax + 1) == 0 and ws(1, 5, kmax) > 0
    buf = (c.c_longlong * 64)()                                   # host memory: every call below returns before it would be read
    p = c.addressof(buf)
    use = lib.glare_vq_usage_i64
    assert use(None, 1, 8, 8, p, p, p, p, 1 << 20, None) == _lib.ERR_INVALID
    assert use(p, 1, 8, 8, None, p, p, p, 1 << 20, None) == _lib.ERR_INVALID
    assert use(p, 1, 8, 8, p, None, p, p, 1 << 20, None) == _lib.ERR_INVALID
    assert use(p, 1, 8, 8, p, p, p, None, 1 << 20, None) == _lib.ERR_INVALID
    for g, n, k in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8)):
        assert use(p, g, n, k, p, p, p, p, 1 << 20, None) == _lib.ERR_INVALID
    assert use(p, 1, 8, kmax + 1, p, p, p, p, 1 << 40, None) == _lib.ERR_UNSUPPORTED
    assert use(p, 65536, 8, 8, p, p, p, p, 1 << 40, None) == _lib.ERR_UNSUPPORTED
    assert use(p, 1, 64 * (2 ** 32 - 1) + 1, 8, p, p, p, p, 1 << 40, None) == _lib.ERR_UNSUPPORTED
    assert use(p, 2, 8, 8, p, p, p, p, ws(2, 8, 8) - 1, None) == _lib.ERR_WORKSPACE
    st = lib.glare_vq_usage_stats
    assert st(None, 1, 8, p, p, p, p, None) == _lib.ERR_INVALID and st(p, 0, 8, p, p, p, p, None) == _lib.ERR_INVALID
    assert st(p, 1, 0, p, p, p, p, None) == _lib.ERR_INVALID and st(p, 1, 8, p, p, p, None, None) == _lib.ERR_INVALID


def test_ops_refuse_cpu_tensors():
    import torch

    from glare_amd import ops

    with pytest.raises(NotImplementedError):
        ops.vq_usage(torch.zeros(8, dtype=torch.int64), 8)
    with pytest.raises(NotImplementedError):
        ops.vq_usage_stats(torch.zeros(1, 8, dtype=torch.int64))
