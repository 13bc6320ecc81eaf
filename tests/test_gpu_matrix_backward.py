"""GPU: the two MFMA kernels behind loss.backward() -- csrc/attn_bwd.hip (fused attention backward and its D = do . o pass) and
csrc/wgrad.hip (weight gradient from the NHWC operands, both entry points) -- with the forward's log-sum-exp (both writers in
csrc/attn.hip) and the materialised pieces softmax2_rows / attention_ds (csrc/train_ops.hip), PER ELEMENT against the fp64
restatements of tests/backward_fp64.py (checked against fp64 autograd and torch's fp64 weight gradient on the CPU:
test_backward_fp64_host.py), in both 16-bit formats.  No element is left out of any comparison.

The rule is the one of fp64_bounds.py:
    16-bit outputs   |got - exact| <= 0.5 ulp16(exact) + slack
    fp32 outputs     |got - exact| <= slack
`slack` is counted from the kernel's own expression and stated next to each call (U = 2^-24, one fp32 rounding): an accumulation of n
products counts n U sum |terms| (one rounding per accumulated product), an elementwise expression its roundings times the magnitudes
of its terms, plus what it reads; a value the kernel rounds to 16 bits on the way (P and dS of the fused backward) enters with
0.5 ulp16 of itself times the operand it multiplies, summed linearly.  Operands are rounded to the 16-bit format before either side
sees them.  Every check goes through tolerances.within(measured / bound, 1.0).

Two families carry the fused backward: random operands (section 4: every rounding counted, small shapes because the linear 16-bit
term hides a single product once N passes ~250) and exact-arithmetic operands (section 5: integer scores, p a power of two, ds
representable, so that the ONLY rounding is the output's and one missing (i, j) term is visible at every size run).  The weight
gradient has the same pair: integer operands that must EQUAL the fp64 sum, and normal operands within the counted bound."""
import functools
import math

import pytest
import torch

import backward_fp64 as R
from fp64_bounds import U, _bits, _f32, _fmt, _r16, _tag, assert_rounded, ulp16
from glare_amd import _lib, ops, train_ops
from glare_amd._lib import check, ptr, stream_handle
from test_gpu_backward_edges import _ratio, check_f32
from tolerances import within

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)
HD = 512


@pytest.fixture(params=("bf16", "fp16"))
def prec(request):
    with ops.use_precision(request.param):
        yield request.param


def _rup(a, b):
    return -(-a // b) * b


def _t(x):
    return x.transpose(-1, -2)


# ---- 2. lse from the forward ------------------------------------------------------------------------------------------------------
def _lse_slack(q64, k64, s, L, N, ks):
    """|lse - L| of attn_fwd_kernel (ks = 1: `m_run + log2(l_tot)`) and attn_combine_kernel (ks > 1: `m + log2(L)`), in log2 units.
    Both evaluate m + log2 sum_j 2^(s'_j - m) with m a lagging running maximum: any m gives the same value, so only these count:
      * s'_j, the score: 32 MFMAs chain 512 products in fp32, 512 U sum_c |q_c| |k_c|; d lse / d s_j = p_j, so sum_j p_j e_s_ij;
      * a term 2^(s'_j - m_run): the subtraction rounds once on |s_j - m_run| <= R (R = the row's spread + 8, m_run lags the maximum
        by at most RESCALE_THR = 8), which the exponential turns into ln 2 U R relative, and v_exp_f32 is good to 1 ulp = 2 U;
      * the running sum (all terms positive, so relative errors add): p0 + p1, the chain of 8 in psum, l_run += psum, one more addition
        per later tile and the exchange with lane ^ 32: 11 + tiles;
      * every rescale (at most one per tile) multiplies l_run by alpha = 2^(m_run - m_new): ln 2 U R + 2 U, and the product: + U;
      * ks > 1: w = 2^(m_s - m) (ln 2 U R + 2 U), w * l_s (U), the chain over the splits (ks U);
      * a relative error r of the sum is r / ln 2 in log2 units; v_log_f32 1 ulp = 2 U on |log2 l| <= 9 + log2 N; the final addition U |lse|."""
    p = torch.exp2(s - L.unsqueeze(-1))
    e_s = 512 * U * (q64.abs() @ _t(k64.abs()))
    R_ = (s.amax(-1) - s.amin(-1)) + 8.0
    tiles = -(-N // 32)
    rel = (LN2 * R_ + 2) + (11 + tiles) + tiles * (LN2 * R_ + 3) + ((LN2 * R_ + 3 + ks) if ks > 1 else 0.0)
    return (p * e_s).sum(-1) + rel * U / LN2 + 2 * U * (9 + math.log2(N)) + U * L.abs()


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("N", (1, 31, 33, 128, 129, 300))
def test_forward_lse_per_row(prec, N, B):
    """ops.attention_d512(..., lse=) at every key split 1..4 the entry point accepts for N (one split per 32-key tile at most): 1 runs
    attn_fwd_kernel's own store, 2..4 attn_combine_kernel's.  Logits: random with a standard deviation of 5 (spread about +-10 to
    +-15: the running maximum is rescaled on the way), and two rows whose maximum sits at key 0 (first tile: everything after it is
    2^-30 of the sum) and at key N - 1 (last tile, possibly ragged: the whole sum so far is rescaled by 2^-30), margin >= 30."""
    g = torch.Generator().manual_seed(N * 10 + B)
    q, k = (torch.randn(B, N, HD, generator=g) * 0.47 for _ in range(2))
    v = torch.randn(B, N, HD, generator=g)
    q[..., :2], k[..., :2] = 0.0, 0.0          # channels 0 and 1 carry the two planted maxima only
    r0, r1 = 0, N - 1
    q[:, r0, 0], k[:, 0, 0] = 9.0, 9.0          # + 81 on (r0, key 0)
    q[:, r1, 1], k[:, N - 1, 1] = 9.0, 9.0      # + 81 on (r1, key N - 1)
    q, k, v = (_r16(t).cuda() for t in (q, k, v))
    q64, k64 = q.double(), k.double()
    s = q64 @ _t(k64)
    _, L = R.attention_fp64(q64, k64, v.double())
    if N > 1:
        for row, key in ((r0, 0), (r1, N - 1)):
            rest = torch.cat([s[:, row, :key], s[:, row, key + 1:]], -1)
            assert int(s[:, row].argmax(-1).min()) == key == int(s[:, row].argmax(-1).max())
            assert float((s[:, row, key] - rest.amax(-1)).min()) >= 30.0
        if N > 3:
            assert float((s[:, 1].amax(-1) - s[:, 1].amin(-1)).min()) > 10.0          # an ordinary row: not near zero
    vt = train_ops.transpose(v, _rup(N, 64))
    ran = []
    for ks in (1, 2, 3, 4):
        lse = torch.full((B, N), float("nan"), dtype=torch.float32, device="cuda")
        if ks > -(-N // 32):          # every split owns at least one key tile
            with pytest.raises(_lib.GlareError):
                ops.attention_d512(q, k, vt, N, key_splits=ks, lse=lse)
            continue
        ops.attention_d512(q, k, vt, N, key_splits=ks, lse=lse)
        check_f32(lse, L, _lse_slack(q64, k64, s, L, N, ks), "lse:%dx%d:ks%d" % (B, N, ks))
        ran.append(ks)
    assert ran == list(range(1, min(4, -(-N // 32)) + 1))


# ---- 3, 4. the fused backward, random operands -----------------------------------------------------------------------------------
def _backward(q, k, v, o, do, lse, ln2_scale):
    """glare_attention_d512_backward_bf16 with a workspace the test owns -> (dq, dk, dv, D): D = the [B, N] floats that
    attn_bwd_dsum_kernel leaves at the start of the workspace"""
    B, N, _ = q.shape
    lib = _lib.lib()
    nws = int(lib.glare_attention_d512_backward_workspace_bytes(B, N))
    assert nws == B * N * 4
    ws = torch.full((B, N), float("nan"), dtype=torch.float32, device="cuda")
    dq, dk, dv = (torch.full_like(q, float("nan")) for _ in range(3))
    check(lib.glare_attention_d512_backward_bf16(ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(dq), ptr(dk), ptr(dv), B, N,
                                                 ln2_scale, ptr(ws), nws, stream_handle()), "glare_attention_d512_backward_bf16")
    return dq, dk, dv, ws


@functools.lru_cache(maxsize=None)
def _random_case(prec_name, B, N):
    """q scaled for base-2 logits of standard deviation 4 (spread about +-8 and more); lse = fp32 of the fp64 L, o = the 16-bit
    rounding of the fp64 O: the same `o` and `lse` go to the kernel and to the reference.  Computed once per case and left unchanged."""
    assert prec_name == ops.precision()
    g = torch.Generator().manual_seed(B * 1000 + N)
    q = torch.randn(B, N, HD, generator=g) * (4.0 / HD ** 0.5)
    k, v, do = (torch.randn(B, N, HD, generator=g) for _ in range(3))
    q, k, v, do = (_r16(t).cuda() for t in (q, k, v, do))
    O, L = R.attention_fp64(q.double(), k.double(), v.double())
    return q, k, v, _r16(O), do, L.float()


def _dsum_tol(o64, do64):
    """attn_bwd_dsum_kernel: a lane's 8 products (exact in fp32 for bf16, one rounding each at worst) and 7 additions, then the 6
    additions of wave_sum: 21 U sum |do| |o|"""
    return 21 * U * (do64.abs() * o64.abs()).sum(-1)


@pytest.mark.parametrize("B,N", R.ATTN_CASES)
def test_dsum_per_row(prec, B, N):
    q, k, v, o, do, lse = _random_case(prec, B, N)
    D = _backward(q, k, v, o, do, lse, LN2)[3]
    o64, do64 = o.double(), do.double()
    check_f32(D, (do64 * o64).sum(-1), _dsum_tol(o64, do64), "dsum:%dx%d" % (B, N))


@pytest.mark.parametrize("B,N", R.ATTN_CASES)
def test_fused_backward_per_element_random_operands(prec, B, N):
    """The slack, from attn_bwd_kernel (x, y: the two score tiles; the same expressions in all three passes):
      s' = x        each wave chains its 256 channels (256 U on its half of sum_c |q_c| |k_c|), the halves are added once (U |s|):
                    e_s = 257 U sum_c |q_c| |k_c|;  dp' = y the same on |do| |v|
      p' = exp2(x - Lq)              the subtraction rounds once on |s| + |L|; v_exp_f32 1 ulp = 2 U:
                    e_p = p (2^(e_s + U (|s| + |L|)) (1 + 2 U) - 1)
      D'            _dsum_tol
      t' = y - Dq   e_t = e_dp + e_D + U (|dp| + |D|)
      ds' = pe * t' * ln2            ln2 ((p + e_p) (|t| + e_t) - p |t|), and two products: 2 U |ds|
      P / dS -> 16 bits              0.5 ulp16(|value| + its error): h = e + 0.5 ulp16
      out = sum over the streamed rows of (P | dS) * T: the error of every term h |T|, summed linearly, and the fp32 accumulation of the
                    32 * tiles products of the chain (rows beyond N multiply zeros): 32 tiles U sum (|value| + h) |T|
    ln2_scale reaches the kernel as a C float; the reference uses that float."""
    q, k, v, o, do, lse = _random_case(prec, B, N)
    dq, dk, dv, D = _backward(q, k, v, o, do, lse, LN2)
    q64, k64, v64, o64, do64, L = (t.double() for t in (q, k, v, o, do, lse))
    ln2 = _f32(LN2)
    s, p, dp, D64, ds = R.attention_backward_terms(q64, k64, v64, o64, do64, L, ln2)
    eq, ek, ev, _ = R.attention_backward_fp64(q64, k64, v64, o64, do64, L, ln2)
    tag = "attn_bwd:%dx%d" % (B, N)
    e_D = _dsum_tol(o64, do64)
    check_f32(D, D64, e_D, tag + ":D")
    arg = 257 * U * (q64.abs() @ _t(k64.abs())) + U * (s.abs() + L.abs().unsqueeze(-1))
    e_p = p * (torch.exp2(arg) * (1 + 2 * U) - 1.0)
    t = dp - D64.unsqueeze(-1)
    e_t = 257 * U * (do64.abs() @ _t(v64.abs())) + e_D.unsqueeze(-1) + U * (dp.abs() + D64.abs().unsqueeze(-1))
    e_ds = ln2 * ((p + e_p) * (t.abs() + e_t) - p * t.abs()) + 2 * U * ds.abs()
    h_p, h_ds = e_p + 0.5 * ulp16(p + e_p), e_ds + 0.5 * ulp16(ds.abs() + e_ds)
    acc = 32 * -(-N // 32) * U
    a_p, a_ds = p + h_p, ds.abs() + h_ds
    assert_rounded(dv, ev, _t(h_p) @ do64.abs() + acc * (_t(a_p) @ do64.abs()), tag + ":dv")
    assert_rounded(dk, ek, _t(h_ds) @ q64.abs() + acc * (_t(a_ds) @ q64.abs()), tag + ":dk")
    assert_rounded(dq, eq, h_ds @ k64.abs() + acc * (a_ds @ k64.abs()), tag + ":dq")
    wdq, wdk, wdv = train_ops.attention_backward_fused(q, k, v, o, do, lse, LN2)          # the wrapper: the same launch
    assert torch.equal(_bits(wdq), _bits(dq)) and torch.equal(_bits(wdk), _bits(dk)) and torch.equal(_bits(wdv), _bits(dv))


# ---- 5. the fused backward, exact-arithmetic operands ------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", R.EXACT_CASES + (R.EXACT_CASE_LARGE,))
def test_fused_backward_exact_operands(prec, B, N):
    """backward_fp64.exact_attention_case: integer scores, an integer `lse` per row that makes p a power of two in [2^-6, 1], integer
    dp and D, ln2_scale = 1.  The entry point does not check that lse and o belong to q, k, v, which is what lets the test choose them.
    Every product and partial sum is then exact in fp32, p and ds are exactly representable in 16 bits, and what is left is
      * v_exp_f32 at an integer argument, allowed its 2 U, and the rounding of pe * t (U): 3 U sum |terms| -- far inside half a
        16-bit ulp of p or ds, so the 16-bit rounding returns the exact value and these vanish on a correct kernel;
      * the output's 16-bit rounding: 0.5 ulp16(exact).
    The condition that makes the family worth running is asserted first, on the reference alone: removing ANY single (i, j) term moves at
    least one output element by more than twice its bound (the host test asserts the same and the exactness of every partial sum for
    all cases but the largest, whose 2.6e8 scores are left to the device)."""
    m, emin = _fmt()
    q, k, v, o, do, L = (t.cuda() for t in R.exact_attention_case(B, N))
    exact, bounds, (p, ds) = R.exact_attention_bounds(q, k, v, o, do, L, m, emin, n_u=3.0)
    sens = float(R.single_term_sensitivity(q, k, do, p, ds, bounds).min())
    assert sens > 2.0, sens
    assert max(float((ds.abs() @ k.abs()).max()), float((_t(ds.abs()) @ q.abs()).max()), float((_t(p) @ do.abs()).max())) / float(p.min()) < 2 ** 24
    del p, ds
    q16, k16, v16, o16, do16 = (_r16(t) for t in (q, k, v, o, do))
    assert all(torch.equal(a.double(), b) for a, b in zip((q16, k16, v16, o16, do16), (q, k, v, o, do)))
    dq, dk, dv, D = _backward(q16, k16, v16, o16, do16, L.float().contiguous(), 1.0)
    tag = "attn_bwd_exact:%dx%d" % (B, N)
    assert torch.equal(D.double(), (do * o).sum(-1)), tag          # an integer sum of two terms: exact
    for got, ex, bd, name in zip((dq, dk, dv), exact, bounds, ("dq", "dk", "dv")):
        assert got.dtype == ops.act_dtype() and got.shape == ex.shape
        within(float(_ratio((got.double() - ex).abs(), bd).max()), 1.0, _tag(tag + ":" + name))
    if (B, N) == R.EXACT_CASE_LARGE:
        del exact, bounds
        torch.cuda.empty_cache()          # gigabytes of fp64 scores: hand them back


# ---- 6. the materialised pieces ----------------------------------------------------------------------------------------------------
PIECE_N = (1, 63, 64, 65, 255, 256, 257, 330)


@pytest.mark.parametrize("n", PIECE_N)
def test_softmax2_rows_per_element(prec, n):
    """softmax2_rows_kernel, one workgroup of 256 per row (n = 256: the workgroup's stride).  Row 0: random logits (standard
    deviation 4); row 1: all equal (P = 1 / n); row 2: one dominant entry, 60 above the rest.  S is a view with a row stride > n.
      e_j = exp2f(s_j - m): the subtraction rounds once (U |s_j - m|, ln 2 of it relative after the exponential), exp2f 1 ulp = 2 U
      sum: a thread's chain of ceil(n / 256) terms, 6 additions of wave_sum, 2 over the waves; all positive, so the terms' relative
           errors (their maximum) and the additions add up relatively
      inv = 1 / sum (U), P = e_j * inv (U); a result below the smallest fp32 normal may be flushed: + 2^-126"""
    rows, ldp = 3, _rup(n + 8, 8)
    g = torch.Generator().manual_seed(n)
    full = torch.randn(rows, n + 5, generator=g) * 4
    full[1, :n] = 1.75
    full[2, n // 2] += 60.0
    full = full.cuda()
    S = full[:, :n]
    assert S.stride(0) > n
    P = train_ops.softmax2_rows(S, n, ldp)
    assert P.shape == (rows, ldp) and int(_bits(P[:, n:]).abs().max()) == 0          # the pad columns: zero bits
    S64 = S.double()
    exact = R.softmax2_rows_fp64(S64)
    d = (S64 - S64.amax(-1, keepdim=True)).abs()
    term = LN2 * U * d + 2 * U
    rel = term + term.amax(-1, keepdim=True) + (-(-n // 256) + 8) * U + 2 * U
    assert_rounded(P[:, :n].contiguous(), exact, exact * rel + 2.0 ** -126, "softmax2:%d" % n)
    assert torch.equal(_bits(P[1, :n]), _bits(P[1, :1]).expand(n))                     # the all-equal row: one value
    assert float(P[2, n // 2]) == 1.0                                                   # the dominant entry


@pytest.mark.parametrize("n", PIECE_N)
def test_attention_ds_per_element(prec, n):
    """attn_ds_kernel, d = 512.  delta = sum_c dO_c O_c: per thread two products and two additions (4), 6 additions of wave_sum, 2
    over the waves: 12 U sum |dO| |O|.  dS = scale * P * (dP - delta): the difference rounds once on |dP| + |delta| and carries delta's
    error, times |scale P|; the two products 2 U |dS|.  dP is a view with a row stride > n; `scale` reaches the kernel as a C float."""
    rows, ldp = 3, _rup(n + 8, 8)
    g = torch.Generator().manual_seed(100 + n)
    P = torch.zeros(rows, ldp)
    P[:, :n] = torch.softmax(torch.randn(rows, n, generator=g) * 3, -1)
    P[:, n:] = 0.5                                                                    # pad columns of P must not reach dS
    dPf = (torch.randn(rows, n + 3, generator=g) * 2).cuda()
    dO, O = (_r16(torch.randn(rows, HD, generator=g)).cuda() for _ in range(2))
    P, dP = _r16(P).cuda(), dPf[:, :n]
    assert dP.stride(0) > n
    dS = train_ops.attention_ds(P, dP, dO, O, n, LN2)
    assert dS.shape == (rows, ldp) and int(_bits(dS[:, n:]).abs().max()) == 0
    scale = _f32(LN2)
    P64, dP64, dO64, O64 = P[:, :n].double(), dP.double(), dO.double(), O.double()
    exact, delta = R.attention_ds_fp64(P64, dP64, dO64, O64, scale)
    e_delta = 12 * U * (dO64.abs() * O64.abs()).sum(-1, keepdim=True)
    slack = scale * P64 * (e_delta + U * (dP64.abs() + delta.abs().unsqueeze(-1))) + 2 * U * exact.abs()
    assert_rounded(dS[:, :n].contiguous(), exact, slack, "attn_ds:%d" % n)


# ---- 7. the weight gradient --------------------------------------------------------------------------------------------------------
# (B, H, W, Ci, Co, pitch, off) -> make_plan's (nks, nstrips, ysplits, rps, S): k-steps of 16 pixels per strip row, strips per image row,
# row ranges per strip, rows per range, partials per group (csrc/wgrad.hip; _plan below restates it and the test confirms each)
WGRAD_CASES = {
    (1, 1, 1, 8, 8, 8, 0): (1, 1, 1, 1, 1),            # a single pixel: all taps but the centre see only padding; one partial, no reduction
    (1, 1, 17, 8, 16, 8, 0): (2, 1, 1, 1, 1),          # one row; a strip of two k-steps, the second holds one pixel
    (2, 3, 15, 16, 8, 24, 8): (1, 1, 1, 3, 2),         # narrower than one k-step; channels at an offset; one partial per image
    (1, 4, 96, 64, 64, 64, 0): (6, 1, 1, 4, 1),        # one strip of the maximum six k-steps: the largest LDS slots
    (1, 4, 97, 16, 16, 16, 0): (1, 7, 1, 4, 7),        # seven strips of 16: the last one owns one pixel
    (1, 9, 33, 72, 136, 80, 8): (3, 1, 3, 3, 3),       # both channel counts ragged over two (three) 64-blocks; bias from ci-block 0 only
    (2, 40, 40, 128, 72, 128, 0): (3, 1, 10, 4, 20),   # ten row ranges per image: their halo rows cross range boundaries
}
GROUPS_CASE = (3, 2, 10, 24, 64, 8)                    # (groups, B, H, W, Ci, Co) of test_conv_weight_gradient_groups
GROUPS_PLAN = (2, 1, 3, 4, 6)                          # three row ranges per image


def _cdiv(a, b):
    return -(-a // b)


def _plan(G, B, H, W, Ci, Co):
    """make_plan of csrc/wgrad.hip: the strip width with the least padding of the row (the fewest strips among equals), then about
    512 workgroups over all tiles and groups in row ranges of at least 4 rows"""
    best, nks, nstrips = 1 << 30, 1, 1
    for ns in range(_cdiv(W, 96), _cdiv(W, 16) + 1):
        ks = _cdiv(_cdiv(W, ns), 16)
        if ks <= 6 and ns * ks * 16 - W < best:
            best, nks, nstrips = ns * ks * 16 - W, ks, ns
    tiles = _cdiv(Ci, 64) * _cdiv(Co, 64) * G * B * nstrips
    ys = min(max(1, _cdiv(512, tiles)), _cdiv(H, 4))
    rps = _cdiv(H, ys)
    ys = _cdiv(H, rps)
    return nks, nstrips, ys, rps, B * nstrips * ys


def _check_plan(ksize, G, B, H, W, Ci, Co, expected):
    lib = _lib.lib()
    assert _plan(G, B, H, W, Ci, Co) == expected
    S, n_out = expected[4], (ksize * ksize * Ci + 1) * Co
    assert int(lib.glare_conv_wgrad_workspace_bytes(ksize, G, B, H, W, Ci, Co)) == (G * S * n_out * 4 if S > 1 else 0)
    if G == 1:
        assert int(lib.glare_conv_wgrad_oihw_workspace_bytes(ksize, B, H, W, Ci, Co)) == S * n_out * 4
    return S


def _wgrad_operands(case, exact):
    """x [B, H, W, pitch] and g [B, H, W, Co + 8] (8 channels the kernel must not read): integers in [-3, 3], every partial and every sum
    an integer below 2^24 (9 * B * H * W <= 28 800), or normal"""
    B, H, W, Ci, Co, pitch, off = case
    gen = torch.Generator().manual_seed(H * 100 + W + Ci)
    if exact:
        x = torch.randint(-3, 4, (B, H, W, pitch), generator=gen).float()
        gy = torch.randint(-3, 4, (B, H, W, Co + 8), generator=gen).float()
        assert 9 * B * H * W < 2 ** 24
    else:
        x, gy = torch.randn(B, H, W, pitch, generator=gen), torch.randn(B, H, W, Co + 8, generator=gen)
    return _r16(x).cuda(), _r16(gy).cuda()


def _rows(dW, db):
    """[Co, Ci, k, k], [Co] -> [(ty, tx, ci) + 1][Co], the NHWC entry point's layout"""
    Co, Ci, k, _ = dW.shape
    return torch.cat([dW.permute(2, 3, 1, 0).reshape(k * k * Ci, Co), db.view(1, Co)], 0)


def _oihw(ksize, x, pitch, off, gy, Ci, Co, dw, ci_off, db):
    """glare_conv_wgrad_oihw_bf16 itself (the wrapper has no pitch / offset of x)"""
    B, H, W, _ = x.shape
    lib = _lib.lib()
    nws = int(lib.glare_conv_wgrad_oihw_workspace_bytes(ksize, B, H, W, Ci, Co))
    ws = torch.full((nws // 4,), float("nan"), dtype=torch.float32, device="cuda")
    check(lib.glare_conv_wgrad_oihw_bf16(ksize, ptr(x), pitch, off, ptr(gy), gy.shape[-1], ptr(dw), dw.shape[1], ci_off, ptr(db), B, H, W, Ci,
                                         Co, ptr(ws), nws, stream_handle()), "glare_conv_wgrad_oihw_bf16")


SENTINEL = -7.25


def _run_both_entry_points(ksize, case, x, gy):
    """-> (NHWC result [k k Ci + 1][Co], OIHW dw [Co][Ci + 16][k][k] filled at ci_off = 8 over a sentinel, db)"""
    B, H, W, Ci, Co, pitch, off = case
    out = torch.full((1, ksize * ksize * Ci + 1, Co), float("nan"), dtype=torch.float32, device="cuda")
    assert train_ops.conv_weight_grad_nhwc(ksize, x, gy, Co, Ci, off, out=out) is out
    dw = torch.full((Co, Ci + 16, ksize, ksize), SENTINEL, dtype=torch.float32, device="cuda")
    db = torch.full((Co,), float("nan"), dtype=torch.float32, device="cuda")
    _oihw(ksize, x, pitch, off, gy, Ci, Co, dw, 8, db)
    dw2 = torch.full_like(dw, SENTINEL)
    _oihw(ksize, x, pitch, off, gy, Ci, Co, dw2, 8, None)                               # db absent
    assert torch.equal(_bits(dw2), _bits(dw))
    outside = torch.cat([dw[:, :8], dw[:, 8 + Ci:]], 1)
    assert torch.equal(_bits(outside), _bits(torch.full_like(outside, SENTINEL)))       # the other sources' channels: bit for bit
    return out[0], dw[:, 8:8 + Ci].contiguous(), db


@pytest.mark.parametrize("ksize", (1, 3))
@pytest.mark.parametrize("case", sorted(WGRAD_CASES))
def test_weight_gradient_exact_operands(prec, case, ksize):
    """Integer operands: dW and db must EQUAL the fp64 sums, through both entry points."""
    B, H, W, Ci, Co, pitch, off = case
    _check_plan(ksize, 1, B, H, W, Ci, Co, WGRAD_CASES[case])
    x, gy = _wgrad_operands(case, exact=True)
    eW, eb = R.conv_weight_grad_fp64(x[..., off:off + Ci].double(), gy[..., :Co].double(), ksize)
    out, dw, db = _run_both_entry_points(ksize, case, x, gy)
    assert torch.equal(out.double(), _rows(eW, eb))
    assert torch.equal(dw.double(), eW) and torch.equal(db.double(), eb)
    if ksize == 3 and H == 1 and W == 1:          # a single pixel: only the centre tap sees it
        centre = torch.zeros(3, 3, dtype=torch.bool, device="cuda")
        centre[1, 1] = True
        assert float(dw[:, :, ~centre].abs().max()) == 0.0 and float(dw[:, :, 1, 1].abs().max()) > 0


@pytest.mark.parametrize("ksize", (1, 3))
@pytest.mark.parametrize("case", sorted(WGRAD_CASES))
def test_weight_gradient_random_operands(prec, case, ksize):
    """Normal operands.  The products of two 16-bit numbers are exact in fp32; an element is the fp32 accumulation of one product per
    pixel of its partial (MFMA chains of 16, row after row) and the ascending chain over the S partials: at most (B H W + S) roundings on
    sum |g| |x| (the bias: on sum |g|, its products with 1).  A second call gives the same bits (fixed order, no atomics)."""
    B, H, W, Ci, Co, pitch, off = case
    S = _check_plan(ksize, 1, B, H, W, Ci, Co, WGRAD_CASES[case])
    x, gy = _wgrad_operands(case, exact=False)
    x64, g64 = x[..., off:off + Ci].double(), gy[..., :Co].double()
    eW, eb = R.conv_weight_grad_fp64(x64, g64, ksize)
    mW, mb = R.conv_weight_grad_fp64(x64.abs(), g64.abs(), ksize)
    n = (B * H * W + S) * U
    out, dw, db = _run_both_entry_points(ksize, case, x, gy)
    tag = "wgrad:k%d:%s" % (ksize, "x".join(str(v) for v in case))
    check_f32(out, _rows(eW, eb), n * _rows(mW, mb), tag + ":nhwc")
    check_f32(dw, eW, n * mW, tag + ":oihw")
    check_f32(db, eb, n * mb, tag + ":db")
    out2, dw2, db2 = _run_both_entry_points(ksize, case, x, gy)
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(dw2), _bits(dw)) and torch.equal(_bits(db2), _bits(db))


@pytest.mark.parametrize("ksize", (1, 3))
def test_weight_gradient_groups_exact_operands(prec, ksize):
    """Three independent filters in one launch, three row ranges per image: groups that walk a leading axis and groups that walk
    channel blocks of one tensor (the two layouts of test_conv_weight_gradient_groups), integer operands, equality."""
    n, B, H, W, Ci, Co = GROUPS_CASE
    _check_plan(ksize, n, B, H, W, Ci, Co, GROUPS_PLAN)
    gen = torch.Generator().manual_seed(70 + ksize)
    x = _r16(torch.randint(-3, 4, (n, B, H, W, Ci), generator=gen).float()).cuda()
    gy = _r16(torch.randint(-3, 4, (n, B, H, W, Co), generator=gen).float()).cuda()
    out = train_ops.conv_weight_grad_nhwc(ksize, x, gy, Co, Ci, groups=n, x_gstride=B * H * W * Ci, g_gstride=B * H * W * Co, shape=(B, H, W))
    xb = x.permute(1, 2, 3, 0, 4).reshape(B, H, W, n * Ci).contiguous()
    gb = gy.permute(1, 2, 3, 0, 4).reshape(B, H, W, n * Co).contiguous()
    outb = train_ops.conv_weight_grad_nhwc(ksize, xb, gb, Co, Ci, groups=n, x_gstride=Ci, g_gstride=Co)
    for grp in range(n):
        eW, eb = R.conv_weight_grad_fp64(x[grp].double(), gy[grp].double(), ksize)
        assert torch.equal(out[grp].double(), _rows(eW, eb)) and torch.equal(outb[grp].double(), _rows(eW, eb))
