"""fp64 restatement of the tile plan's blend weights and of the blend (glare_amd.enhance.plan_axis / axis_weights,
glare_harness_tile_blend_f32), written from the contract and sharing no code with the product, plus the error bound of the fp32 kernel.

The bound.  Per output value the kernel adds at most 9 terms fmaf(wy_i * wx_j, v_ij, acc): v in [0, 1], and the exact weights of an
axis are positive and sum to 1, so every partial sum is at most 1 (+ rounding).  Against the exact sum, each term carries
  - the table rounding of its two weights (each fp64 -> fp32 once): relative 2 * 2^-24 on a term, 2 * 2^-24 absolute over the sum;
  - the rounding of the product wy * wx: relative 2^-24, 2^-24 absolute over the sum;
  - the rounding of the fma's result, at most 2^-24 each (|acc| <= 1 + eps): 9 * 2^-24.
12 * 2^-24 with second-order terms far below one more unit: |acc - acc64| <= 16 * 2^-24 absolute."""
import numpy as np

BOUND = 16 * 2.0 ** -24
U8_CAP = 0.005          # at most this share of the uint8 values may sit so close to a quantisation step that +-1 is allowed


def axis_plan(L, T, O):
    """Window starts and length of one axis (no precondition on T and O: the kernel tests also use ramps narrower than 16)."""
    if L <= T:
        total = 16 - L % 16
        p1 = total // 2                       # auto_padding: the odd pixel goes to the far side, a multiple of 16 gets 8 + 8
        return [-p1], L + total
    stride = T - O
    n = -((L - O) // -stride)
    return [min(i * stride, L - T) for i in range(n)], T


def axis_weights64(L, starts, T, O):
    """fp64 [n][L]: the normalised weight of window i at image coordinate x, 0 where the window does not cover x."""
    n = len(starts)
    w = np.zeros((n, L), dtype=np.float64)
    for x in range(L):
        for i, s in enumerate(starts):
            if s <= x < s + T:
                r = 1.0
                if i > 0:
                    r = min(r, (x + 0.5 - s) / O)
                if i < n - 1:
                    r = min(r, (s + T - x - 0.5) / O)
                w[i, x] = r
    return w / w.sum(axis=0, keepdims=True)


def blend64(tiles, ys, xs, H, W, th, tw, O):
    """tiles: float array [len(ys) * len(xs)][3][th][tw] (any float dtype, inf / NaN allowed) -> (acc64 [H][W][3], count): the blend
    of the clamped windows (NaN -> 0) with exact weights, and the raw inf / NaN values at positions inside the image, once per window."""
    t = np.asarray(tiles, dtype=np.float64)
    wy, wx = axis_weights64(H, ys, th, O), axis_weights64(W, xs, tw, O)
    acc = np.zeros((H, W, 3), dtype=np.float64)
    bad = 0
    for i, y0 in enumerate(ys):
        ya, yb = max(y0, 0), min(y0 + th, H)
        for j, x0 in enumerate(xs):
            xa, xb = max(x0, 0), min(x0 + tw, W)
            raw = t[i * len(xs) + j][:, ya - y0:yb - y0, xa - x0:xb - x0]
            bad += int((~np.isfinite(raw)).sum())
            v = np.clip(np.where(np.isnan(raw), 0.0, raw), 0.0, 1.0)
            acc[ya:yb, xa:xb] += (wy[i, ya:yb, None] * wx[j, None, xa:xb])[:, :, None] * v.transpose(1, 2, 0)
    return acc, bad


def u8_mismatch(u8, acc64):
    """The uint8 rule: u8 == floor(min(acc64, 1) * 255) except where acc64 * 255 lies within 255 * BOUND of an integer, where +-1 is
    allowed -> (number of values breaking the rule, share of values that used the exception)."""
    s = np.minimum(acc64, 1.0) * 255.0
    want = np.floor(s).astype(np.int64)
    d = np.asarray(u8).astype(np.int64) - want
    near = np.abs(s - np.rint(s)) <= 255.0 * BOUND
    wrong = (d != 0) & ~(near & (np.abs(d) == 1))
    return int(wrong.sum()), float(((d != 0) & near).sum()) / d.size
