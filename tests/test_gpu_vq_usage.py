"""GPU: the codebook-usage kernels (csrc/vq_usage.hip) through the C ABI and through glare_amd.ops, against tests/usage_fp64.py.

Counts, `active`, `tokens` and `out_of_range` are integers and must be EQUAL to the restatement.  Entropy and perplexity are fp64 from the
exact counts: each term p log(p + 1e-10) carries a division, an addition, a log (<= 1 ulp) and a product, the K terms are added in some
order, and exp (<= 1 ulp) follows -- relative error of the perplexity (= absolute error of the entropy) <= (K + 8) * 2^-53 * (1 + sum |terms|),
usage_fp64.perplexity_bound.  Shapes: one token; one below, at and one above the span a workgroup histograms; groups whose length is no
multiple of anything; K = 1, 37, 8192 and a K above the single-pass LDS tier; every token on one code; every code once; indices -1, K
and 2^40 mixed in, with guard cells around every output."""
import numpy as np
import pytest
import torch

import usage_fp64 as U
from glare_amd import _lib, metrics, ops
from glare_amd._lib import ptr, stream_handle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = _lib.constants()
TIER, SPAN, KMAX = C["GLARE_VQ_USAGE_TIER"], C["GLARE_VQ_USAGE_SPAN"], C["GLARE_VQ_USAGE_MAX_CODES"]
GUARD = 64                       # int64 cells (and x 8 bytes of workspace) on either side of every output
SENTINEL = -0x0123456789ABCDEF

# (groups, tokens per group, codes, kind)
SHAPES = [(1, 1, 8192, "rand"), (1, SPAN - 1, 8192, "rand"), (1, SPAN, 8192, "rand"), (1, SPAN + 1, 8192, "rand"), (3, 97, 37, "rand"),
          (2, 50, 1, "rand"), (2, 2 * SPAN + 5, 37, "rand"), (2, SPAN + 3, TIER + 37, "rand"), (1, 3000, 8192, "one_code"),
          (1, 8192, 8192, "every_code_once"), (1, TIER + 37, TIER + 37, "every_code_once"), (3, 97, 37, "out_of_range"),
          (2, SPAN + 1, TIER + 37, "out_of_range"), (1, 5, 1, "out_of_range")]


def _indices(G, n, K, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "one_code":
        return np.full((G, n), K - 3, np.int64)
    if kind == "every_code_once":
        return np.stack([rng.permutation(K)[:n] for _ in range(G)]).astype(np.int64)
    idx = rng.integers(0, K, (G, n), dtype=np.int64)
    if kind == "out_of_range":
        bad = np.array([-1, K, 2 ** 40, -2 ** 40, K + TIER, -K - 1, 2 ** 63 - 1, -2 ** 63, 2 ** 32, 2 ** 32 + 1], np.int64)
        where = rng.random((G, n)) < 0.3
        where[:, 0] = True                               # the first and the last token of every group among them
        where[:, -1] = True
        idx[where] = rng.choice(bad, int(where.sum()))
    return idx


def _guarded(cells, fill=SENTINEL):
    buf = torch.full((GUARD + cells + GUARD,), fill, dtype=torch.int64, device=DEV)
    return buf, buf.data_ptr() + GUARD * 8


def _guards_intact(buf, cells):
    b = buf.cpu().numpy()
    return bool((b[:GUARD] == SENTINEL).all() and (b[GUARD + cells:] == SENTINEL).all())


def _abi_usage(idx, K, total0):
    """One glare_vq_usage_i64 call on numpy int64 [G, n] -> (counts, out_of_range, total) as numpy, every output between guard cells."""
    lib = _lib.main_lib()
    G, n = idx.shape
    d = torch.from_numpy(idx).to(DEV)
    counts, pc = _guarded(G * K)
    oor, po = _guarded(G)
    total, pt = _guarded(K)
    total[GUARD:GUARD + K] = torch.from_numpy(total0).to(DEV)
    nws = lib.glare_vq_usage_workspace_bytes(G, n, K)
    assert nws > 0 and nws % 4 == 0
    cells = (nws + 7) // 8
    ws, pw = _guarded(cells)
    _lib.check(lib.glare_vq_usage_i64(ptr(d), G, n, K, pc, po, pt, pw, nws, stream_handle()), "glare_vq_usage_i64")
    torch.cuda.synchronize()
    assert _guards_intact(counts, G * K) and _guards_intact(oor, G) and _guards_intact(total, K), "an output's guard cells were written"
    wsb = ws.cpu().numpy()
    assert (wsb[:GUARD] == SENTINEL).all() and (wsb[GUARD + cells:] == SENTINEL).all(), "the workspace's guard cells were written"
    return (counts[GUARD:GUARD + G * K].view(G, K).cpu().numpy(), oor[GUARD:GUARD + G].cpu().numpy(), total[GUARD:GUARD + K].cpu().numpy())


def _abi_stats(rows):
    lib = _lib.main_lib()
    R, K = rows.shape
    d = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
    tokens, pt = _guarded(R)
    active, pa = _guarded(R)
    ent = torch.full((R + 2,), -7.0, dtype=torch.float64, device=DEV)
    per = torch.full((R + 2,), -7.0, dtype=torch.float64, device=DEV)
    _lib.check(lib.glare_vq_usage_stats(ptr(d), R, K, pt, pa, ent.data_ptr() + 8, per.data_ptr() + 8, stream_handle()), "glare_vq_usage_stats")
    torch.cuda.synchronize()
    assert _guards_intact(tokens, R) and _guards_intact(active, R)
    e, p = ent.cpu().numpy(), per.cpu().numpy()
    assert e[0] == e[-1] == p[0] == p[-1] == -7.0
    return tokens[GUARD:GUARD + R].cpu().numpy(), active[GUARD:GUARD + R].cpu().numpy(), e[1:-1], p[1:-1]


def _assert_stats(rows, got, tag):
    tokens, active, ent, per = got
    K = rows.shape[1]
    for r, row in enumerate(rows):
        want = U.stats(row)
        assert int(tokens[r]) == want["tokens"] and int(active[r]) == want["active"], (tag, r)
        bound = U.perplexity_bound(K, want["abs_terms"])
        rel = abs(float(per[r]) - want["perplexity"]) / want["perplexity"]
        err_h = abs(float(ent[r]) - want["entropy"])
        print("%s row %d: tokens %d active %d perplexity %.17g want %.17g rel %.3g entropy err %.3g bound %.3g"
              % (tag, r, want["tokens"], want["active"], float(per[r]), want["perplexity"], rel, err_h, bound))
        assert np.isfinite(per[r]) and np.isfinite(ent[r])
        assert rel <= bound and err_h <= bound, (tag, r, rel, err_h, bound)


@pytest.mark.parametrize("G,n,K,kind", SHAPES, ids=["%dx%d-K%d-%s" % s for s in SHAPES])
def test_usage_matches_the_restatement(G, n, K, kind):
    idx = _indices(G, n, K, kind, seed=G * 1000 + n + K)
    want_counts, want_oor = U.counts(idx, K, G)
    if kind == "one_code":
        assert want_counts[0, K - 3] == n                    # maximal contention on one LDS cell
    if kind == "every_code_once" and n == K:
        assert (want_counts == 1).all()
    if kind == "out_of_range":
        assert (want_oor > 0).all()
    total0 = np.random.default_rng(7).integers(0, 2 ** 40, K, dtype=np.int64)          # the call ADDS to the total
    counts, oor, total = _abi_usage(idx, K, total0)
    assert np.array_equal(counts, want_counts) and np.array_equal(oor, want_oor)
    assert np.array_equal(total, total0 + want_counts.sum(0))
    assert int(counts.sum()) + int(oor.sum()) == G * n
    # the Python surface: the same numbers, a fresh total, and a given one added to
    d = torch.from_numpy(idx).to(DEV)
    c2, o2, t2 = ops.vq_usage(d.view(-1), K, groups=G)
    assert c2.dtype == o2.dtype == t2.dtype == torch.int64 and tuple(c2.shape) == (G, K) and tuple(o2.shape) == (G,) and tuple(t2.shape) == (K,)
    assert np.array_equal(c2.cpu().numpy(), want_counts) and np.array_equal(o2.cpu().numpy(), want_oor)
    assert np.array_equal(t2.cpu().numpy(), want_counts.sum(0))
    given = torch.from_numpy(total0).to(DEV)
    _, _, t3 = ops.vq_usage(d, K, groups=G, total=given)
    assert t3 is given and np.array_equal(given.cpu().numpy(), total0 + want_counts.sum(0))
    # the statistics of the per-group rows and of the total
    rows = np.concatenate([want_counts, want_counts.sum(0, keepdims=True)])
    _assert_stats(rows, _abi_stats(rows), "abi %s" % kind)
    tk, ac, en, pe = ops.vq_usage_stats(torch.from_numpy(rows).to(DEV))
    assert tk.dtype == ac.dtype == torch.int64 and en.dtype == pe.dtype == torch.float64 and tuple(pe.shape) == (G + 1,)
    _assert_stats(rows, tuple(t.cpu().numpy() for t in (tk, ac, en, pe)), "ops %s" % kind)
    one = ops.vq_usage_stats(torch.from_numpy(rows[-1]).to(DEV))                       # a [K] histogram: 0-d results
    assert all(t.dim() == 0 for t in one) and int(one[0]) == int(rows[-1].sum()) and float(one[3]) == float(pe[-1])


def test_two_calls_into_one_total_equal_one_call_on_the_concatenation():
    K = 8192
    a, b = _indices(2, SPAN + 9, K, "out_of_range", 1), _indices(3, 97, K, "rand", 2)
    total = torch.zeros(K, dtype=torch.int64, device=DEV)
    ops.vq_usage(torch.from_numpy(a).to(DEV), K, groups=2, total=total)
    ops.vq_usage(torch.from_numpy(b).to(DEV), K, groups=3, total=total)
    both = np.concatenate([a.ravel(), b.ravel()])
    c1, o1, t1 = ops.vq_usage(torch.from_numpy(both).to(DEV), K)
    assert torch.equal(total, t1) and torch.equal(c1[0], t1)
    assert np.array_equal(t1.cpu().numpy(), U.counts(both, K)[0][0]) and int(o1[0]) == int(U.counts(both, K)[1][0])


def test_three_launches_give_identical_bytes():
    K = TIER + 37
    idx = torch.from_numpy(_indices(3, 2 * SPAN + 1, K, "out_of_range", 5)).to(DEV)
    runs = []
    for _ in range(3):
        c, o, t = ops.vq_usage(idx, K, groups=3)
        s = ops.vq_usage_stats(torch.cat([c, t[None]]))
        runs.append([x.cpu().numpy().tobytes() for x in (c, o, t) + s])
    assert runs[0] == runs[1] == runs[2]


def test_a_row_without_tokens_has_perplexity_one():
    rows = np.zeros((3, 37), np.int64)
    rows[1, 5] = 4
    tokens, active, ent, per = _abi_stats(rows)
    assert tokens.tolist() == [0, 4, 0] and active.tolist() == [0, 1, 0]
    assert per[0] == 1.0 and per[2] == 1.0 and ent[0] == 0.0 and ent[2] == 0.0 and not np.isnan(per).any()
    _assert_stats(rows, (tokens, active, ent, per), "empty rows")
    # every index out of range: a histogram of zeros
    c, o, t = ops.vq_usage(torch.full((10,), -1, dtype=torch.int64, device=DEV), 37)
    assert int(c.sum()) == 0 and int(o[0]) == 10 and float(ops.vq_usage_stats(t)[3]) == 1.0


def test_bad_arguments_return_their_status_and_write_nothing():
    lib = _lib.main_lib()
    K, n = 37, 100
    idx = torch.zeros(n, dtype=torch.int64, device=DEV)
    counts, pc = _guarded(K)
    oor, po = _guarded(1)
    total, pt = _guarded(K)
    nws = lib.glare_vq_usage_workspace_bytes(1, n, K)
    ws, pw = _guarded((nws + 7) // 8)
    use, s = lib.glare_vq_usage_i64, stream_handle()
    assert use(None, 1, n, K, pc, po, pt, pw, nws, s) == _lib.ERR_INVALID
    assert use(ptr(idx), 1, n, K, None, po, pt, pw, nws, s) == _lib.ERR_INVALID
    assert use(ptr(idx), 1, n, K, pc, None, pt, pw, nws, s) == _lib.ERR_INVALID
    assert use(ptr(idx), 1, n, K, pc, po, pt, None, nws, s) == _lib.ERR_INVALID
    assert use(ptr(idx), 0, n, K, pc, po, pt, pw, nws, s) == _lib.ERR_INVALID
    assert use(ptr(idx), 1, 0, K, pc, po, pt, pw, nws, s) == _lib.ERR_INVALID
    assert use(ptr(idx), 1, n, 0, pc, po, pt, pw, nws, s) == _lib.ERR_INVALID
    assert use(ptr(idx), 1, n, K, pc, po, pt, pw, nws - 1, s) == _lib.ERR_WORKSPACE
    assert use(ptr(idx), 1, n, KMAX + 1, pc, po, pt, pw, 1 << 40, s) == _lib.ERR_UNSUPPORTED          # the stated limit on K
    assert use(ptr(idx), 65536, 1, K, pc, po, pt, pw, 1 << 40, s) == _lib.ERR_UNSUPPORTED
    st = lib.glare_vq_usage_stats
    assert st(None, 1, K, pt, pt, pt, pt, s) == _lib.ERR_INVALID and st(pc, 0, K, pt, pt, pt, pt, s) == _lib.ERR_INVALID
    assert st(pc, 1, 0, pt, pt, pt, pt, s) == _lib.ERR_INVALID and st(pc, 1, K, pt, None, pt, pt, s) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    for buf in (counts, oor, total, ws):
        assert (buf == SENTINEL).all()
    with pytest.raises(_lib.GlareError) as e:
        ops.vq_usage(idx, KMAX + 1)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    assert use(ptr(idx), 1, n, K, pc, po, None, pw, nws, s) == 0                  # the total is optional
    torch.cuda.synchronize()
    assert counts[GUARD:GUARD + K].tolist() == [n] + [0] * (K - 1) and int(oor[GUARD]) == 0 and (total == SENTINEL).all()


def test_codebook_usage_accumulates_resets_and_reports():
    K = 8192
    usage = metrics.CodebookUsage(K, DEV)
    a, b = _indices(2, 375, K, "rand", 11), _indices(1, 100, K, "out_of_range", 12)
    c, o = usage.update(torch.from_numpy(a).to(DEV), groups=2)
    assert np.array_equal(c.cpu().numpy(), U.counts(a, K, 2)[0]) and o.tolist() == [0, 0]
    usage.update(torch.from_numpy(b).to(DEV))
    both = np.concatenate([a.ravel(), b.ravel()])
    want_counts, want_oor = U.counts(both, K)
    want = U.stats(want_counts[0])
    assert usage.counts().dtype == torch.int64 and np.array_equal(usage.counts().cpu().numpy(), want_counts[0])
    s = usage.stats()
    assert set(s) == {"tokens", "active", "active_fraction", "perplexity", "out_of_range"}
    assert s["tokens"] == want["tokens"] and s["active"] == want["active"] and s["active_fraction"] == want["active"] / K
    assert s["out_of_range"] == int(want_oor[0]) > 0
    assert abs(s["perplexity"] - want["perplexity"]) <= U.perplexity_bound(K, want["abs_terms"]) * want["perplexity"]
    usage.discard(c[1])
    assert np.array_equal(usage.counts().cpu().numpy(), want_counts[0] - U.counts(a[1], K)[0][0])
    usage.reset()
    assert usage.stats() == {"tokens": 0, "active": 0, "active_fraction": 0.0, "perplexity": 1.0, "out_of_range": 0}
