"""GPU: the codebook layer's training kernels (csrc/vq_train.hip) through the C ABI, PER ELEMENT against fp64 computed here
(np.add.at on float64), on the indices glare_vq_nearest_f32 returns.

Every bound is derived from the rounding count of the kernels' source (-ffp-contract=off: what is written is what rounds), not
measured.  u = 2^-24 (one fp32 rounding, relative), gamma_n = n u / (1 - n u):
    S      = sum_i (zq_i - z_i)^2                  |err| <= gamma_n sum t_i,   n = 3N + 3: a subtraction and a square form each term,
                                                   and any order of the additions rounds a term at most (terms - 1) times
    dE[k]  = c_e sum_{idx_i = k} (zq_i - z_i)      |err| <= gamma_n |c_e| sum |zq_i - z_i|,  n = (tokens of k) + 3: the subtraction,
                                                   the additions, and c_e = float(2 w_e / 3N) * gl times the sum (three roundings)
    dz[i]  = g_i + c_z (z_i - zq_i)                |err| <= 2^-21 (|g| + |c_z (z - zq)|): float(2 w_z / 3N), times gl, the
                                                   subtraction, the product, the addition -- five roundings, 5 u < 2^-21
A code that no token selected gets exactly 0.0."""
import numpy as np
import pytest
import torch

from glare_amd import _lib, ops
from glare_amd._lib import ptr, stream_handle
from tolerances import within

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = "cuda:0"
BETA = 0.25


def _gamma(n):
    return n * U / (1.0 - n * U)


def _launch(z, E, g, gl, w_z, w_e):
    """numpy fp32 in -> dict of numpy results of one forward + backward through the C ABI."""
    lib = _lib.lib()
    N, K = z.shape[0], E.shape[0]
    zd, Ed, gd = (torch.from_numpy(a).to(DEV).contiguous() for a in (z, E, g))
    gld = torch.tensor([gl], dtype=torch.float32, device=DEV)
    idx = torch.empty(N, dtype=torch.int64, device=DEV)
    zq, st, dz = torch.empty_like(zd), torch.empty_like(zd), torch.empty_like(zd)
    s = torch.empty(1, dtype=torch.float32, device=DEV)
    de = torch.full((K, 3), 7.0, dtype=torch.float32, device=DEV)
    _lib.check(lib.glare_vq_nearest_f32(ptr(zd), ptr(Ed), N, K, 3, ptr(idx), ptr(zq), stream_handle()), "glare_vq_nearest_f32")
    nws = lib.glare_vq_train_workspace_bytes(N, K)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    _lib.check(lib.glare_vq_loss_sum_f32(ptr(zd), ptr(zq), N, 3, ptr(st), ptr(s), ptr(ws), nws, stream_handle()), "glare_vq_loss_sum_f32")
    _lib.check(lib.glare_vq_backward_f32(ptr(zd), ptr(zq), ptr(idx), ptr(gd), ptr(gld), N, K, 3, 2.0 * w_z / (3 * N), 2.0 * w_e / (3 * N),
                                         ptr(dz), ptr(de), ptr(ws), nws, stream_handle()), "glare_vq_backward_f32")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in (("idx", idx), ("zq", zq), ("st", st), ("S", s), ("dz", dz), ("dE", de))}


def _check(z, E, g, gl, w_z, w_e, tag):
    N, K = z.shape[0], E.shape[0]
    r = _launch(z, E, g, gl, w_z, w_e)
    idx = r["idx"]
    # the indices are vq_nearest's, bit for bit, and z_q the selected rows
    ridx, rzq = ops.vq_nearest(torch.from_numpy(z).to(DEV), torch.from_numpy(E).to(DEV))
    assert np.array_equal(idx, ridx.cpu().numpy()) and np.array_equal(r["zq"], rzq.cpu().numpy())
    assert idx.min() >= 0 and idx.max() < K and np.array_equal(r["zq"], E[idx])
    z64, zq64, g64, gl64 = z.astype(np.float64), E[idx].astype(np.float64), g.astype(np.float64), float(np.float32(gl))
    d = zq64 - z64
    # the straight-through output: z + (zq - z), two fp32 roundings spelled
    assert np.array_equal(r["st"], (z + (E[idx] - z)).astype(np.float32))
    # S
    terms = d * d
    within(abs(float(r["S"][0]) - terms.sum()) / max(_gamma(3 * N + 3) * terms.sum(), 1e-300), 1.0, tag + ":S")
    # dz
    cz = gl64 * (2.0 * w_z / (3 * N))
    t = cz * (z64 - zq64)
    bound = 2.0 ** -21 * (np.abs(g64) + np.abs(t)) + 1e-45
    within(float((np.abs(r["dz"].astype(np.float64) - (g64 + t)) / bound).max()), 1.0, tag + ":dz")
    # dE
    ce = gl64 * (2.0 * w_e / (3 * N))
    acc, mag = np.zeros((K, 3)), np.zeros((K, 3))
    np.add.at(acc, idx, d)
    np.add.at(mag, idx, np.abs(d))
    count = np.bincount(idx, minlength=K)
    used = count > 0
    de = r["dE"].astype(np.float64)
    assert np.all(r["dE"][~used] == 0.0) and not np.signbit(r["dE"][~used]).any()          # exactly 0.0
    if used.any():
        bound = _gamma(count[used] + 3)[:, None] * abs(ce) * mag[used] + 1e-45
        within(float((np.abs(de[used] - ce * acc[used]) / bound).max()), 1.0, tag + ":dE")
    # bitwise reproducible: a second launch on the same inputs
    r2 = _launch(z, E, g, gl, w_z, w_e)
    for k in ("S", "dz", "dE", "st"):
        assert np.array_equal(r[k].view(np.int32), r2[k].view(np.int32)), k
    return r, count


def _draw(N, K, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal((K, 3)).astype(np.float32),
            rng.standard_normal((N, 3)).astype(np.float32))


# one token, one code; below / at / above a wave; the first size with several token tiles and segments (4097 = 8 x 512 + 1); the
# segment count at its cap of 32 (N > 16 384), several 512-token tiles per segment, a ragged last one
@pytest.mark.parametrize("N,K", [(1, 1), (63, 5), (64, 8192), (65, 8192), (4097, 8192), (25600, 8192)])
@pytest.mark.parametrize("legacy", [False, True])
def test_loss_sum_and_gradients_per_element(N, K, legacy):
    z, E, g = _draw(N, K, N + K)
    w_z, w_e = (1.0, BETA) if legacy else (BETA, 1.0)
    _, count = _check(z, E, g, 1.0 if N < 100 else 65536.0, w_z, w_e, "%dx%d:%s" % (N, K, "legacy" if legacy else "plain"))
    if K == 8192 and N <= 4097:
        assert (count == 0).sum() >= K - N                 # most codes unused: their rows are exactly 0 (checked above)


def test_one_code_owns_every_token():
    """The skew the per-code sum must not care about: 4097 tokens, all on code 3 of 8192."""
    rng = np.random.default_rng(7)
    E = (rng.standard_normal((8192, 3)) * 0.1 + 50.0).astype(np.float32)
    E[3] = (0.3, -0.2, 0.1)
    z = (E[3] + 0.05 * rng.standard_normal((4097, 3))).astype(np.float32)
    r, count = _check(z, E, rng.standard_normal((4097, 3)).astype(np.float32), -3.0, BETA, 1.0, "skew")
    assert count[3] == 4097 and np.all(r["idx"] == 3)


def test_duplicate_code_rows_lowest_index_wins():
    """Exact ties: rows 2 / 5 / 9 identical -> every token of theirs goes to row 2, and dE to that row only."""
    z, E, g = _draw(2000, 16, 11)
    E[5] = E[2]
    E[9] = E[2]
    r, count = _check(z, E, g, 2.0, 1.0, BETA, "ties")
    assert count[2] > 0 and count[5] == 0 and count[9] == 0
    assert np.all(r["dE"][5] == 0.0) and np.all(r["dE"][9] == 0.0) and np.any(r["dE"][2] != 0.0)


def test_autograd_node_returns_the_search_indices():
    from glare_amd import autograd as A

    z, E, _ = _draw(700, 300, 5)
    zd = torch.from_numpy(z).to(DEV).view(1, 28, 25, 3).requires_grad_(True)
    Ed = torch.from_numpy(E).to(DEV).requires_grad_(True)
    st, loss, idx = A.vq_straight_through(zd, Ed, BETA, 1.0)
    ridx, rzq = ops.vq_nearest(torch.from_numpy(z).to(DEV), torch.from_numpy(E).to(DEV))
    assert torch.equal(idx, ridx) and not idx.requires_grad and st.shape == zd.shape
    d = rzq.double().cpu() - torch.from_numpy(z).double()
    assert abs(float(loss.detach()) - 1.25 * float((d * d).mean())) <= _gamma(2100 + 6) * 1.25 * float((d * d).mean())
    (st.sum() + loss).backward()
    assert zd.grad.shape == zd.shape and Ed.grad.shape == Ed.shape and bool(torch.isfinite(zd.grad).all())


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.lib()
    N, K = 600, 40
    z, E, g = (torch.from_numpy(a).to(DEV) for a in _draw(N, K, 3))
    idx, zq = ops.vq_nearest(z, E)
    gl = torch.ones(1, device=DEV)
    nws = lib.glare_vq_train_workspace_bytes(N, K)
    assert nws >= 2 * K * 3 * 4 and lib.glare_vq_train_workspace_bytes(0, K) == 0
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    s = torch.full((1,), -5.0, device=DEV)
    st, dz, de = (torch.full(shape, -5.0, device=DEV) for shape in ((N, 3), (N, 3), (K, 3)))
    st_ = stream_handle()
    I, W, UNS = _lib.ERR_INVALID, _lib.ERR_WORKSPACE, _lib.ERR_UNSUPPORTED
    assert lib.glare_vq_loss_sum_f32(None, ptr(zq), N, 3, ptr(st), ptr(s), ptr(ws), nws, st_) == I
    assert lib.glare_vq_loss_sum_f32(ptr(z), None, N, 3, ptr(st), ptr(s), ptr(ws), nws, st_) == I
    assert lib.glare_vq_loss_sum_f32(ptr(z), ptr(zq), N, 3, ptr(st), None, ptr(ws), nws, st_) == I
    assert lib.glare_vq_loss_sum_f32(ptr(z), ptr(zq), N, 3, ptr(st), ptr(s), None, nws, st_) == I
    assert lib.glare_vq_loss_sum_f32(ptr(z), ptr(zq), 0, 3, ptr(st), ptr(s), ptr(ws), nws, st_) == I
    assert lib.glare_vq_loss_sum_f32(ptr(z), ptr(zq), N, 4, ptr(st), ptr(s), ptr(ws), nws, st_) == UNS
    assert lib.glare_vq_loss_sum_f32(ptr(z), ptr(zq), N, 3, ptr(st), ptr(s), ptr(ws), 3, st_) == W
    cz = ce = 1.0 / (3 * N)
    args = lambda **kw: [kw.get(k, v) for k, v in (("z", ptr(z)), ("zq", ptr(zq)), ("idx", ptr(idx)), ("g", ptr(g)), ("gl", ptr(gl)), ("N", N),
                                                   ("K", K), ("dim", 3), ("cz", cz), ("ce", ce), ("dz", ptr(dz)), ("dE", ptr(de)),
                                                   ("ws", ptr(ws)), ("nws", nws), ("stream", st_))]
    for bad in ({"z": None}, {"zq": None}, {"idx": None}, {"gl": None}, {"N": 0}, {"K": 0}, {"dz": None, "dE": None}, {"ws": None}):
        assert lib.glare_vq_backward_f32(*args(**bad)) == I, bad
    assert lib.glare_vq_backward_f32(*args(dim=2)) == UNS
    assert lib.glare_vq_backward_f32(*args(nws=nws - 1)) == W
    torch.cuda.synchronize()
    for t in (s, st, dz, de):                                      # nothing was launched: every output still holds its fill
        assert bool((t == -5.0).all())
    # a NULL upstream gradient of the straight-through output is zero, and either gradient may be left out
    assert lib.glare_vq_backward_f32(*args(g=None, dE=None)) == 0 and lib.glare_vq_backward_f32(*args(dz=None)) == 0
    torch.cuda.synchronize()
    want = (gl.double() * cz).float() * (z - zq)
    assert torch.equal(dz, want) and bool((de != -5.0).all())
