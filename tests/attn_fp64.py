"""The forward attention OUTPUT restated in plain fp64 torch: the reference of test_gpu_attn_edges.py (csrc/attn.hip: attn_fwd_kernel behind
ops.attention_d512, attn_kv_fwd_kernel behind ops.attention_kv512, attn_combine_kernel behind both when the keys are split).  Written
from the header of attn.hip,
    out[b, i, :] = sum_j softmax2_j(q_i . k_j) v_j          base 2, the scale and log2 e folded into q by the caller
    d512 form:  q, k [B, N, 512], v_t [B, 512, v_pitch] (V transposed; columns N .. v_pitch - 1 are pad)
    kv512 form: q, x [B, N, 512], keys AND values are x
and checked against torch.softmax in test_attn_fp64_host.py.  A plain module like tolerances.py.

Three more things live here, each used by the CPU test and by the GPU test alike:

REPLAY (replay): the kernels' ORDER of operations in fp32 -- 32-key tiles; the running maximum with the deferred rescale, taken only when
some row of the 32-row wave exceeds m_run + 8 (the branch is wave-uniform: rows that did not grow are rescaled too, by 2^(m_run - m_new));
p rounded to the 16-bit format for the P.V product but summed UNROUNDED into l; key-split partials (O, m, l) merged as attn_combine_kernel
does.  It is not the reference.  It exists to count the roundings of out_slack below, to prove the exact family exact, and to carry the
mutations that only exist in the order of operations (a skipped rescale, l from rounded p, a dropped split weight).

EXACT FAMILY (exact_case): operands with which the replay in fp32 gives the fp64 result bit for bit, in both formats, so that the only
rounding left in the kernel is the output's.  It rests on v_exp_f32 being exact at integer arguments -- the property
backward_fp64.exact_attention_case already relies on (its p are powers of two as well) -- and on these choices:
  * row i asks channels 2i and 2i + 1 only (q = 1 and 128 there), so s_ij = k_j[2i] + 128 k_j[2i + 1] is ANY integer matrix we like, with
    |k| <= 64 a number of both formats; in the kv form the same tensor is the value, in the d512 form v holds integers in [-3, 3];
  * a row's SURVIVORS sit at M - d_j, d_j in [0, 7], with sum_j 2^-d_j a power of two: l is then a power of two, 1 / l and O / l are exact, and
    the numerator sum_j 2^-d_j v_j needs at most 7 + 8 + 7 bits.  Every other key is at least 1100 below M, so that its weight is 0 in fp32
    (anything 200 below would do for that) AND in fp64: at 200 below, fp64 keeps 2^-200 v_j, which turns an exact zero of the output into
    -0 or +0 by the sign of v_j, and the expected bits would depend on it;
  * the members: a power-of-two count of keys at M (d = 0); 2^r keys at M - r in earlier tiles and 1 or 3 at M in a later one -- the maximum
    rises by r <= 7, the rescale is DEFERRED and p = 2^r there, unless a neighbour of the wave triggers in that tile, in which case it is TAKEN
    with alpha = 2^-r.  (A rise the kernel defers needs a key at M - r, whose weight is not 0: a power-of-two COUNT at the maximum alone cannot
    reach that branch with a visible result, the SUM of the weights must be the power of two.  r = 8 would need 256 keys at M - 8, more than the
    largest N here: the family reaches p = 2^7, the staircase row of the random family p = 2^7.5.)  Rises of more than 8 (floor -> M, and
    -1200 -> -1150 -> M in every other wave) take the rescale with alpha = 2^-1150 = 0; what they wipe may be inexact, 0 x finite is 0;
  * the tile of the jump moves with the wave and the image, so maxima sit in the last, partial tile (the last valid key included) and the
    partial maxima of key splits differ (weights 2^(m_s - m) of 0, 2^-r and 1).

SLACK (slack_terms): |got - exact| <= 0.5 ulp16(exact) + slack for the 16-bit output, counted from the source (U = 2^-24, u16 = 2^-(m+1) the
relative half ulp of the format, p_j the exact softmax weight, A_d = sum_j p_j |v_jd|, D_d = sum_j p_j |v_jd - out_d|, R the row's score
spread + 8 = the largest |s_j - m_run|).  An error e_j of score j moves out_d by ln 2 p_j (v_jd - out_d) e_j, and a relative error of a weight
that the numerator and l SHARE by p_j (v_jd - out_d) times it -- hence D_d, which is 0 where one key holds all the weight:
  score     32 MFMAs chain 512 products in fp32: e_s = 512 U sum_c |q_c| |k_c|;  ln 2 sum_j p_j e_s |v_jd - out_d|
  exp       s_j - m_run rounds once (ln 2 U R after the exponential) and v_exp_f32 is good to 1 ulp = 2 U, shared:  (ln 2 R + 2) U D_d
  p16       the P.V product takes p rounded to 16 bits, l does NOT (the mismatch): nothing cancels and the weight is |v_jd|, u16 A_d -- a
            rounding shared with l would leave u16 D_d; `mismatch` = u16 |out_d| is the part that l from rounded p would remove
  underflow p relative to m_run below the format's normal range (fp16: 2^-14) rounds absolutely, 2^(emin - m - 1), and v_exp_f32 flushes below
            2^-126; m_run trails the final maximum M by 8 at most and never leads it, so in units of 2^(s_j - M) the error is no larger:
            (2^(emin - m - 1) + 2^-126) sum_{j: 2^(s_j - M) < 2^emin} |v_jd| / l
  O         fp32 accumulation of 32 products per tile: 32 tiles U A_d; one rescale per tile at most, each alpha = 2^(m_run - m_new) with the
            error of `exp` (it re-weights old against new keys: x D_d) and one product rounding on O (U A_d) and on l (U |out_d|)
  l         p0 + p1, the chain of 8, l_run += psum, one addition per later tile, the exchange with lane ^ 32: (11 + tiles) U |out_d|
  final     1 / l (counted as v_rcp_f32's 1 ulp, 2 U) and the product: 3 U |out_d|
  combine   per split w = 2^(m_s - m) (`exp` again, x D_d), the fmaf (U A_d), w l_s and the sum (2 U |out_d|)
In bf16 p16 is the term that counts (u16 = 2^-9 against e_s of about 2^-10 on the random family); in fp16 (u16 = 2^-12) the worst-case chain of
`score` is the largest term.
The pair form's hi + lo is an fp32-class value: the slack alone plus the rounding of lo = round16(value - hi) (conv_fp64.pair_slack)."""
import math

import torch

from conv_fp64 import U, binade_extra, fmt, pair_slack, ulp16  # noqa: F401  (re-exported for the two test files)

HD, BN, WAVE_ROWS, BM = 512, 32, 32, 128
RESCALE_THR = 8.0
LN2 = math.log(2.0)
NS = (1, 31, 32, 33, 64, 65, 127, 128, 129, 161)
BS = (1, 3)
FLOOR, FLOOR2 = -1200, -1150


def tiles(N):
    return -(-N // BN)


def splits_of(N):
    """every key split 1..4 the entry points accept for N: each owns at least one tile"""
    return tuple(range(1, min(4, tiles(N)) + 1))


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def attention_fp64(q, k, v, mutate=None, pad=0.0):
    """q, k, v [B, N, 512] fp64 -> out [B, N, 512].  `mutate` names ONE deliberate error (the sensitivity checks of
    test_attn_fp64_host.py); None is the operation.  pad: what column N of the values holds (kv form: the zeros behind the descriptor's
    range; d512 form: the V^T pad, the largest finite number in test_gpu_attn_edges.py)."""
    B, N, _ = q.shape
    if mutate == "query_of_next_image":          # the last row of every image's last query block reads row N of the allocation
        q = q.clone()
        q[:, N - 1] = q.roll(-1, 0)[:, 0]
    s = q @ k.transpose(-1, -2)
    if mutate == "key_past_n":                   # key N: zeros behind the descriptor's range, score 0, value `pad`
        s = torch.cat([s, torch.zeros(B, N, 1, dtype=s.dtype)], -1)
        v = torch.cat([v, torch.full((B, 1, HD), pad, dtype=v.dtype)], 1)
    elif mutate == "last_key_masked":
        s = s.clone()
        s[..., N - 1] = -math.inf
    elif mutate == "tile_dropped":               # the last tile that is not the only one, else the only one but its first key
        s = s.clone()
        t = tiles(N) - 1
        s[..., max(t * BN, 1):] = -math.inf
    elif mutate == "v_column_shifted":           # keys of the last tile take the value of the next column (the last one the first pad column, 0)
        v = v.clone()
        t0 = (tiles(N) - 1) * BN
        v[:, t0:] = torch.cat([v[:, t0 + 1:], torch.zeros(B, 1, HD, dtype=v.dtype)], 1)
    e = torch.exp2(s - s.amax(-1, keepdim=True))
    return (e / e.sum(-1, keepdim=True)) @ v


def v_of_vt(v_t, N):
    """[B, 512, v_pitch] -> the N valid columns as [B, N, 512]"""
    return v_t[:, :, :N].transpose(1, 2)


PAD_D512 = 65504.0          # the largest finite fp16 number (a number of bf16's range as well)


def attention_d512_fp64(q, k, v_t, N, mutate=None):
    return attention_fp64(q, k, v_of_vt(v_t, N), mutate, PAD_D512)


def attention_kv512_fp64(q, x, mutate=None):
    return attention_fp64(q, x, x, mutate)


# ---- the replay -------------------------------------------------------------------------------------------------------------------------
def _exp2f(x):
    """v_exp_f32 as an fp32 function: exact at integers, else the correctly rounded value (the instruction is good to 1 ulp)"""
    return torch.exp2(x.double()).float()


def replay(q, k, v, dtype, ks=1, mutate=None):
    """The kernels' order of operations in fp32 on [B, N, 512] operands that are numbers of `dtype` -> dict:
    value (fp32, before the output's rounding), hi, lo (`dtype`), and per row: `taken` (rescales that changed its maximum after its split's
    first tile), `forced` (of those, rises of 8 or less that a neighbour of the wave forced), `deferred` (tiles whose maximum exceeded
    m_run without a rescale), `pmax` (largest p), `last` (its largest score sits in the last tile)."""
    B, N, _ = q.shape
    T, G = tiles(N), -(-N // WAVE_ROWS)
    rows = G * WAVE_ROWS
    s = torch.zeros(B, rows, T * BN, dtype=torch.float32)
    s[:, :N, :N] = (q.double() @ k.double().transpose(-1, -2)).float()          # rows past N: q reads as 0
    s[:, :, N:] = -math.inf                                                     # `if (kv >= p.N) s[r] = -inf`
    vp = torch.zeros(B, T * BN, HD, dtype=torch.float32)                        # rows past N: 0 x a finite pad
    vp[:, :N] = v.float()
    stat = {n: torch.zeros(B, rows) for n in ("taken", "forced", "deferred", "pmax")}
    stat["last"] = (s.argmax(-1) >= (T - 1) * BN).float()
    parts = []
    for sp in range(ks):
        t0, t1 = T * sp // ks, T * (sp + 1) // ks
        m = torch.full((B, rows), -1e30, dtype=torch.float32)
        l = torch.zeros(B, rows, dtype=torch.float32)
        O = torch.zeros(B, rows, HD, dtype=torch.float32)
        for t in range(t0, t1):
            st = s[:, :, t * BN:(t + 1) * BN]
            mx = st.amax(-1)
            trig = (mx > m + RESCALE_THR).view(B, G, WAVE_ROWS).any(-1, keepdim=True).expand(B, G, WAVE_ROWS).reshape(B, rows)
            m_new = torch.maximum(m, mx)
            alpha = torch.where(trig, _exp2f(m - m_new), torch.ones_like(m))
            grew = trig & (m_new > m)
            if t > t0:
                stat["taken"] += grew.float()
                stat["forced"] += (grew & (m_new - m <= RESCALE_THR)).float()
                stat["deferred"] += ((mx > m) & ~trig).float()
            l = l * alpha
            a_o = alpha.clone()
            if mutate == "rescale_skipped" and t > t0:          # row 0 of every wave keeps its accumulators as they were
                a_o.view(B, G, WAVE_ROWS)[:, :, 0] = 1.0
            O = O * a_o.unsqueeze(-1)
            m = torch.where(trig, m_new, m)
            p = _exp2f(st - m.unsqueeze(-1))
            stat["pmax"] = torch.maximum(stat["pmax"], p.amax(-1))
            p16 = p.to(dtype).float()
            l = l + (p16 if mutate == "l_from_rounded_p" else p).sum(-1)
            O = O + p16 @ vp[:, t * BN:(t + 1) * BN]
        parts.append((O, m, l))
    if ks == 1:
        O, m, l = parts[0]
        value = O * (1.0 / l).unsqueeze(-1)
    else:
        mm = torch.full((B, rows), -1e30, dtype=torch.float32)
        for _, m, _ in parts:
            mm = torch.maximum(mm, m)
        acc, L = torch.zeros(B, rows, HD, dtype=torch.float64), torch.zeros(B, rows, dtype=torch.float32)
        for sp, (O, m, l) in enumerate(parts):
            w = _exp2f(m - mm)
            if mutate == "split_weight_dropped" and sp == 0:
                w = torch.ones_like(w)
            L = L + w * l
            acc = (w.double().unsqueeze(-1) * O.double() + acc).float().double()          # fmaf: one rounding
        value = acc.float() * (1.0 / L).unsqueeze(-1)
    value = value[:, :N]
    hi = value.to(dtype)
    out = {"value": value, "hi": hi, "lo": (value - hi.float()).to(dtype)}
    out.update({n: t[:, :N] for n, t in stat.items()})
    return out


# ---- the exact family -------------------------------------------------------------------------------------------------------------------
def exact_scores(B, N):
    """-> the integer score matrix [B, N, N] of the exact family (the module's docstring has the members)"""
    T = tiles(N)
    i_, j_ = torch.arange(N).view(N, 1), torch.arange(N).view(1, N)
    S = (FLOOR - (i_ + j_) % 4).double().repeat(B, 1, 1)
    for b in range(B):
        for i in range(N):
            g, kind = i // WAVE_ROWS, i % 4
            M = -float((i + b) % 4)
            J = (g + b) % T
            lo_, hi_ = J * BN, min(N, J * BN + BN)
            Lj = hi_ - lo_
            if kind == 3 and (g + b) % 2 == 1 and J < T - 1:          # a second jump of more than 8: this wave's neighbours are rescaled in tile J + 1
                S[b, i, lo_ + i % Lj] = FLOOR2
                hi2 = min(N, (J + 1) * BN + BN)
                S[b, i, hi2 - 2:hi2] = M
            elif kind in (0, 3):                                     # a power-of-two count at M, all in the tile of the jump
                n = 1 << ((i // 4) % 3)
                while n > Lj:
                    n //= 2
                for u in range(n):
                    S[b, i, lo_ + (i + u) % Lj] = M
            else:                                                    # 2^r keys at M - r, then n at M with n + 1 a power of two
                J2 = T - 1 if kind == 1 else min(J + 1, T - 1)
                n = 1 if (i // 8) % 2 else 3
                r = 1 + (i // 4) % 7
                if J2 > J:
                    avail = (J2 - J) * BN
                    lo2, hi2 = J2 * BN, min(N, J2 * BN + BN)
                    n = n if hi2 - lo2 >= n else 1
                else:
                    avail, hi2 = Lj, hi_
                    while n > 0 and n + 1 > Lj:          # one tile holds both sets: 2^r + n keys
                        n //= 2
                    avail = Lj - n
                while (1 << r) > avail:
                    r -= 1
                if n == 0:                               # one key in the tile: it is the maximum
                    S[b, i, lo_] = M
                    continue
                S[b, i, lo_:lo_ + (1 << r)] = M - r
                S[b, i, hi2 - n:hi2] = M
    return S


def exact_case(B, N, form):
    """-> (q, k, v) [B, N, 512] fp64, integer valued; form "kv": k and v are the same tensor"""
    assert 2 * N <= HD
    S = exact_scores(B, N)
    coarse = torch.round(S / 128.0)
    fine = S - 128.0 * coarse
    assert float(fine.abs().max()) <= 64 and float(coarse.abs().max()) <= 64
    r = torch.arange(B * N).view(B, N, 1)
    c = torch.arange(HD).view(1, 1, HD)
    k = ((5 * r + 3 * c) % 7 - 3).double()                 # the channels no row asks: small integers that differ with key and channel
    k[:, :, 0:2 * N:2] = fine.transpose(1, 2)              # k_j[2i] = fine_ij
    k[:, :, 1:2 * N:2] = coarse.transpose(1, 2)
    q = torch.zeros(B, N, HD, dtype=torch.float64)
    idx = torch.arange(N)
    q[:, idx, 2 * idx], q[:, idx, 2 * idx + 1] = 1.0, 128.0
    assert torch.equal(q @ k.transpose(1, 2), S)
    v = k if form == "kv" else ((37 * r + 11 * c + (r * c) % 13) % 7 - 3).double()
    return q, k, v


# ---- the random family ------------------------------------------------------------------------------------------------------------------
def structured_rows(N):
    """(staircase, dominant key N - 1, dominant key 0) -- rows of the random family that carry a planted profile (N >= 4)"""
    return (1, N // 2, N - 1) if N >= 4 else ()


def random_case(B, N, form, dtype):
    """Base-2 logits of standard deviation 4, per-channel offsets on V (the operands of test_gpu_attn_schedule.py), rounded to `dtype`;
    channels 0..2 of q and k carry three planted rows and are 0 elsewhere in q:
      staircase   no random part; key 5 of tile t sits at the sum of t steps of alternately 7.5 (deferred) and 8.5 (taken), every other key at 0
      last        + 64 on key N - 1: a dominant key in the last tile, alone there when N % 32 == 1
      first       + 64 on key 0: a dominant key in tile 0, everything after it far below"""
    g = torch.Generator().manual_seed(7000 + 10 * N + B + (100000 if form == "kv" else 0))
    off = torch.linspace(-1, 1, HD)
    if form == "kv":
        q = torch.randn(B, N, HD, generator=g) * 0.153          # 4 / sqrt(512 (1 + 1 / 3))
        k = torch.randn(B, N, HD, generator=g) + off
        v = k
    else:
        q = torch.randn(B, N, HD, generator=g) * 0.42           # sqrt(4 / sqrt(512))
        k = torch.randn(B, N, HD, generator=g) * 0.42
        v = torch.randn(B, N, HD, generator=g) + off
    q[..., :3], k[..., :3] = 0.0, 0.0
    rows = structured_rows(N)
    if rows:
        a, b_, c_ = rows
        q[:, a] = 0.0
        q[:, a, 0] = 0.5
        level = 0.0
        for t in range(tiles(N)):
            if t * BN + 5 < N:
                k[:, t * BN + 5, 0] = 2.0 * level
            level += 7.5 if t % 2 == 0 else 8.5
        q[:, b_, 1], k[:, N - 1, 1] = 8.0, 8.0
        q[:, c_, 2], k[:, 0, 2] = 8.0, 8.0
    q, k, v = (t.to(dtype).double() for t in (q, k, v))
    return q, (v if form == "kv" else k), v


# ---- the slack --------------------------------------------------------------------------------------------------------------------------
def slack_terms(q, k, v, dtype):
    """-> (exact out, f, mismatch): f(ks) is the slack [B, N, 512] fp64 at `ks` key splits; the terms are the module's docstring"""
    mb, emin = fmt(dtype)
    u16 = 2.0 ** -(mb + 1)
    B, N, _ = q.shape
    T = tiles(N)
    s = q @ k.transpose(-1, -2)
    P = torch.exp2(s - s.amax(-1, keepdim=True))
    l = P.sum(-1, keepdim=True)
    p = P / l
    out, va = p @ v, v.abs()
    A, ao = p @ va, out.abs()
    R = (s.amax(-1, keepdim=True) - s.amin(-1, keepdim=True)) + RESCALE_THR
    eps = (LN2 * R + 2.0) * U
    pe = p * (HD * U * (q.abs() @ k.abs().transpose(-1, -2)))
    D, Ds = torch.empty_like(out), torch.empty_like(out)
    for b in range(B):          # [N, N, 512] at a time
        dev = (v[b].unsqueeze(0) - out[b].unsqueeze(1)).abs()
        D[b] = (p[b].unsqueeze(1) @ dev).squeeze(1)
        Ds[b] = (pe[b].unsqueeze(1) @ dev).squeeze(1)
    under = (2.0 ** (emin - mb - 1) + 2.0 ** -126) * ((P < 2.0 ** emin).double() @ va) / l
    base = LN2 * Ds + eps * D + u16 * A + under + BN * T * U * A + T * (eps * D + U * (A + ao)) + (11 + T) * U * ao + 3 * U * ao
    comb = eps * D + U * A + 2 * U * ao
    return out, (lambda ks: base + (ks * comb if ks > 1 else 0.0)), u16 * ao


def out_slack(q, k, v, ks, dtype):
    out, f, mismatch = slack_terms(q, k, v, dtype)
    return out, f(ks), mismatch


def ratio16(got64, exact, slack, dtype):
    """|got - exact| / (0.5 ulp16(exact) + slack), the value the kernel rounds allowed into the next binade (conv_fp64.binade_extra)"""
    return (got64 - exact).abs() / (0.5 * ulp16(exact, dtype) + slack + binade_extra(exact, slack, dtype))


def ratio_pair(hi_plus_lo64, exact, slack, dtype):
    return (hi_plus_lo64 - exact).abs() / (slack + pair_slack(exact, slack, dtype))
