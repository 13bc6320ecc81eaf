"""fp64 numpy restatement of NIQE as glare_amd.metrics.niqe specifies it (Mittal et al. 2013, evaluated as basicsr's calculate_niqe:
BT.601 luma rounded to integers, two scales, 96 x 96 blocks, 36 features per block, Mahalanobis-like distance to a pristine model),
step by step, and the synthetic pristine model the tests use.  Written from the published algorithm; nothing here imports the product.
A plain module like fp64_bounds.py.

`storage=np.float32` reruns the restatement the way the published implementation stores its arrays at the second scale: there its
image comes out of imresize as float32, so scipy's convolve returns mu and window (*) y^2 as float32 and the squares, their difference,
sigma and n are float32 numpy arithmetic (the first scale is float64 there and stays float64 here).  Its deviation from the fp64 run is
that implementation's own noise: the bar of tests/test_gpu_niqe.py."""
import math

import numpy as np

BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], dtype=np.float64) / 256
GRID = 0.2 + 0.001 * np.arange(9801)          # 0.2, 0.201, ..., 10.000


def synthetic_params(seed=5):
    """The pristine model of the tests: seeded mu, cov = A A^T / 36 + 0.01 I, the window a normalised 7 x 7 Gaussian of sigma 7 / 6."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.2, 2.0, 36)
    A = rng.standard_normal((36, 36))
    ax = np.arange(7, dtype=np.float64) - 3
    g = np.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / (2 * (7.0 / 6.0) ** 2))
    return {"mu_pris_param": mu, "cov_pris_param": A @ A.T / 36 + 0.01 * np.eye(36), "gaussian_window": g / g.sum()}


def luma_numerator(rgb_u8):
    """65481 R + 128553 G + 24966 B as exact integers: y = 16 + numerator / 255000."""
    c = np.asarray(rgb_u8).astype(np.int64)
    return 65481 * c[..., 0] + 128553 * c[..., 1] + 24966 * c[..., 2]


def luma(rgb_u8):
    """16 + round(numerator / 255000), ties to even, in integer arithmetic -> int64."""
    q, rem = np.divmod(luma_numerator(rgb_u8), 255000)
    return 16 + q + ((rem > 127500) | ((rem == 127500) & (q % 2 == 1)))


def crop(y):
    return y[..., :y.shape[-2] // BLOCK * BLOCK, :y.shape[-1] // BLOCK * BLOCK]


def convolve_nearest(y, window):
    """scipy.ndimage.convolve(y, window, mode='nearest') for a 7 x 7 window, in fp64: out[i, j] = sum w[a, b] y[i + 3 - a, j + 3 - b]."""
    y = np.asarray(y, dtype=np.float64)
    H, W = y.shape
    p = np.pad(y, 3, mode="edge")
    out = np.zeros((H, W), dtype=np.float64)
    for a in range(7):
        for b in range(7):
            out += window[a, b] * p[6 - a:6 - a + H, 6 - b:6 - b + W]
    return out


def window_sums(window):
    """(s0, 1 - s0) of the window.  A window normalised in fp64 sums to 1 only to within its own rounding (49 weights of 2^-53 relative
    each), so a sum within 2^-50 of 1 is 1: the statistics of a flat region are then exactly those of real arithmetic."""
    s0 = math.fsum(np.asarray(window, dtype=np.float64).ravel().tolist())
    return (1.0, 0.0) if abs(1.0 - s0) <= 2.0 ** -50 else (s0, 1.0 - s0)


def mscn(y, window, storage=np.float64):
    """n = (y - mu) / (sigma + 1), mu = window (*) y, sigma = sqrt |window (*) y^2 - mu^2|.

    fp64: the local moments are taken about the pixel's own value c (d = y - c, S1 = sum w d, S2 = sum w d^2; y - mu = c (1 - s0) - S1,
    var = S2 - S1^2 + (1 - s0) (c^2 s0 + 2 c S1)), which is the same in real numbers.  NIQE counts the SIGNS of n: window (*) y^2 - mu^2
    formed directly leaves +-1e-14 in fp64 where the real result is 0 (a flat region), and such a pixel would be counted on a side
    that rounding chose.  About c a flat region gives exactly 0, as real arithmetic does.
    storage=np.float32: the direct form on float32 arrays, as the published implementation computes its second scale."""
    if storage is np.float64:
        y = np.asarray(y, dtype=np.float64)
        H, W = y.shape
        s0, oms0 = window_sums(window)
        p = np.pad(y, 3, mode="edge")
        S1, S2 = np.zeros((H, W)), np.zeros((H, W))
        for a in range(7):
            for b in range(7):
                d = p[6 - a:6 - a + H, 6 - b:6 - b + W] - y
                S1 += window[a, b] * d
                S2 += window[a, b] * d * d
        var = S2 - S1 * S1 + oms0 * (y * y * s0 + 2 * y * S1)
        return (y * oms0 - S1) / (np.sqrt(np.abs(var)) + 1)
    y = np.asarray(y, dtype=np.float64).astype(storage)
    mu = convolve_nearest(y, window).astype(storage)
    second = convolve_nearest((y * y).astype(np.float64), window).astype(storage)
    sigma = np.sqrt(np.abs(second - mu * mu))
    n = (y - mu) / (sigma + storage(1))
    assert n.dtype == storage
    return n.astype(np.float64)


def halve(y):
    """imresize(y, 0.5, antialiasing=True) for even sizes: the 8 taps over inputs 2 j - 3 .. 2 j + 4, edges reflected including the edge
    pixel; the H pass, then the W pass."""
    y = np.asarray(y, dtype=np.float64)
    for axis in (0, 1):
        L = y.shape[axis]
        assert L % 2 == 0 and L >= 4, y.shape
        idx = 2 * np.arange(L // 2)[:, None] - 3 + np.arange(8)[None, :]
        idx = np.where(idx < 0, -idx - 1, idx)
        idx = np.where(idx >= L, 2 * L - 1 - idx, idx)
        y = np.tensordot(np.take(y, idx, axis=axis), TAPS, axes=([axis + 1], [0]))      # take: the 8 inputs of an output on axis + 1
    return y


def block_maps(block):
    """The five maps of one block of n: itself and its product with each circular in-block shift."""
    return [block] + [block * np.roll(block, s, axis=(0, 1)) for s in SHIFTS]


def map_moments(v):
    """{count(v < 0), count(v > 0), sum_{v<0} v^2, sum_{v>0} v^2, sum |v|} of one map."""
    neg, pos = v[v < 0], v[v > 0]
    return np.array([neg.size, pos.size, math.fsum(neg * neg), math.fsum(pos * pos), math.fsum(np.abs(v).ravel())], dtype=np.float64)


def block_moments(n, bh=BLOCK, bw=BLOCK):
    """[W / bw][H / bh][5][5]: blocks column-major, maps, moments."""
    H, W = n.shape
    out = np.zeros((W // bw, H // bh, 5, 5), dtype=np.float64)
    for bx in range(W // bw):
        for by in range(H // bh):
            for m, v in enumerate(block_maps(n[by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw])):
                out[bx, by, m] = map_moments(v)
    return out


def _rho(g):
    return math.gamma(2 / g) ** 2 / (math.gamma(1 / g) * math.gamma(3 / g))


RHO = np.array([_rho(g) for g in GRID])


def aggd(moments, count):
    """One map's (alpha, beta_l, beta_r, grid index) from its five moments and its element count."""
    cn, cp, sn, sp, sa = (float(x) for x in moments)
    with np.errstate(all="ignore"):
        left = np.sqrt(np.float64(sn) / np.float64(cn))
        right = np.sqrt(np.float64(sp) / np.float64(cp))
        gamma = left / right
        rhat = (np.float64(sa) / count) ** 2 / ((np.float64(sn) + np.float64(sp)) / count)
        R = rhat * (gamma ** 3 + 1) * (gamma + 1) / (gamma ** 2 + 1) ** 2
        k = int(np.argmin((RHO - R) ** 2))          # the first on ties; a NaN everywhere is index 0, as numpy has it
        alpha = float(GRID[k])
        scale = math.sqrt(math.gamma(1 / alpha) / math.gamma(3 / alpha))
        return alpha, float(left * scale), float(right * scale), k


def features_from_moments(moments, count):
    """[..., 5, 5] moments of blocks of `count` elements -> ([..., 18] features, [..., 5] grid indices)."""
    moments = np.asarray(moments, dtype=np.float64)
    lead = moments.shape[:-2]
    flat = moments.reshape(-1, 5, 5)
    feats, ks = np.zeros((flat.shape[0], 18)), np.zeros((flat.shape[0], 5), dtype=np.int64)
    for i, blockm in enumerate(flat):
        row = []
        for m in range(5):
            alpha, bl, br, k = aggd(blockm[m], count)
            ks[i, m] = k
            if m == 0:
                row += [alpha, (bl + br) / 2]
            else:
                row += [alpha, (br - bl) * math.gamma(2 / alpha) / math.gamma(1 / alpha), bl, br]
        feats[i] = row
    return feats.reshape(lead + (18,)), ks.reshape(lead + (5,))


def score_from_features(feats36, params):
    """[n_blocks, 36] -> (score, None) or (None, reason)."""
    feats36 = np.asarray(feats36, dtype=np.float64)
    good = feats36[~np.isnan(feats36).any(axis=1)]
    if good.shape[0] < 2:
        return None, "fewer than 2 blocks without NaN features"
    with np.errstate(all="ignore"):
        mu_d = np.nanmean(feats36, axis=0)
    cov_d = np.cov(good, rowvar=False)
    d = np.asarray(params["mu_pris_param"], dtype=np.float64).reshape(36) - mu_d
    inv = np.linalg.pinv((np.asarray(params["cov_pris_param"], dtype=np.float64) + cov_d) / 2)
    return float(np.sqrt(d @ inv @ d)), None


def scale_images(img_u8, storage=np.float64):
    """[(y, block size)] of the two scales of one uint8 RGB image, or None when it has fewer than 2 whole blocks."""
    y = crop(luma(img_u8)).astype(np.float64)
    if (y.shape[0] // BLOCK) * (y.shape[1] // BLOCK) < 2:
        return None
    y2 = halve(y / 255.0) * 255.0
    return [(y, BLOCK), (y2.astype(storage).astype(np.float64), BLOCK // 2)]


def features(img_u8, params, storage=np.float64):
    """[n_blocks, 36] or None."""
    scales = scale_images(img_u8, storage)
    if scales is None:
        return None
    cols = []
    for s, (y, b) in enumerate(scales):
        n = mscn(y, params["gaussian_window"], storage if s == 1 else np.float64)
        cols.append(features_from_moments(block_moments(n, b, b), b * b)[0].reshape(-1, 18))
    return np.concatenate(cols, axis=1)


def niqe(img_u8, params, storage=np.float64):
    """The whole score of one uint8 RGB image: a float, or None (fewer than 2 whole blocks, or fewer than 2 NaN-free rows)."""
    f = features(img_u8, params, storage)
    return None if f is None else score_from_features(f, params)[0]
