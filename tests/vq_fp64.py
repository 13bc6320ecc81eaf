"""The codebook search (csrc/vq.hip, ops.vq_nearest) restated for test_gpu_vq_edges.py, with the input families that make the search decide
something.  A plain module like tolerances.py; checked on the CPU by test_vq_scoring_fp64_host.py.

What is restated
  launch shape   slots_for(n): the kernel's token lanes per workgroup (64 up to 32 768 tokens, 128 up to 65 536, 256 above), parts = 1024 / slots
                 code ranges, range p of a resident chunk of nc codes = [nc p / parts, nc (p + 1) / parts); chunks of 8192 codes.
  search         search_f32(): the kernel's fp32 distance -- zz = (z0 z0 + z1 z1) + z2 z2, ee alike, dot = fma(z2, e2, fma(z1, e1, z0 e0)),
                 d = (zz + ee) - 2 dot -- per code range, the first minimum inside a range, the ranges merged by (distance, index).  It exists to
                 carry MUTATIONS (what a wrong kernel would do); the bit reference of the GPU test is the C oracle, not this.
  fp64 check     excess(): per token (d64(z, cb[idx]) - min_k d64(z, cb[k])) / (C_ROUND U ((zz + ee_chosen) + (zz + ee_best))), over ALL codes, on
                 any device, in slices.  Independent of the oracle, which shares the kernel's spelling.

The count C_ROUND = 8, from vq.hip:50-75, per side (the chosen code and the true nearest one), in units of U (zz + ee):
  zz, ee   a product, then two additions on the path of the first term: 3 roundings each, all terms non-negative   3
  zz + ee  one addition                                                                                            1
  dot      a product and two fma links on sum |z_i e_i| <= (zz + ee) / 2, doubled exactly                          3
  d        the subtraction rounds |d| = |z - e|^2; for the two codes compared here -- the nearest and one the kernel preferred to it -- d is
           the SMALL distance, below zz + ee unless the token lies opposite every code                              1
The kernel chose c over the true nearest b because its computed d_c <= its computed d_b, so d64_c - d64_b <= err_c + err_b.
"""
import functools
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

U = 2.0 ** -24
C_ROUND = 8
CHUNK = 8192               # VQ_CHUNK: codes resident in LDS at once
THREADS = 1024             # VQ_THREADS
TPT = 2                    # VQ_TPT

SMALL_N = (1, 127, 128, 129)
# 65 537 + 511 = 129 x 512 fills its last 256-lane workgroup exactly; 65 537 + 510 leaves it one token short
LARGE_N = (32767, 32768, 32769, 65535, 65536, 65537, 65537 + 510, 65537 + 511)
SMALL_K = (8192, 1000, 7, 3, 1, 8193, 16385)
LARGE_K = (8192, 1000, 8193)
FAMILIES = ("random", "midpoint0.7", "midpoint30", "midpoint_shifted", "duplicate", "special")
SHIFT = (40.0, -25.0, 60.0)          # the shifted codebook: zz + ee ~ 1e4, the distances to a neighbour ~ 1e-2


def slots_for(n_tokens):
    """glare_vq_nearest_f32's token lanes per workgroup"""
    lanes = (n_tokens + TPT - 1) // TPT
    slots = ((lanes + 255) // 256 + 63) // 64 * 64
    slots = max(slots, 64)
    return THREADS // 4 if slots > 128 else slots


def parts_for(n_tokens):
    return THREADS // slots_for(n_tokens)


def ranges(nc, parts):
    """[(lo, hi)] of the parts' shares of a resident chunk of nc codes"""
    return [(nc * p // parts, nc * (p + 1) // parts) for p in range(parts)]


def range_of(c, n_codes, parts):
    """(chunk, part) that scans code c"""
    chunk, r = divmod(c, CHUNK)
    nc = min(CHUNK, n_codes - chunk * CHUNK)
    for p, (lo, hi) in enumerate(ranges(nc, parts)):
        if lo <= r < hi:
            return chunk, p
    raise AssertionError("code %d of %d is in no range of %d parts" % (c, n_codes, parts))


# ---- families ----------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) % (2 ** 31))


@functools.lru_cache(maxsize=None)
def codebook(k, scale=0.7, shifted=False, seed=0):
    cb = _rng("cb", k, scale, shifted, seed).randn(k, 3) * scale
    if shifted:
        cb = cb + np.asarray(SHIFT)
    cb = cb.astype(np.float32)
    cb.setflags(write=False)
    return cb


def nearest_neighbour(cb, rows):
    """for the codes `rows` the index of the nearest OTHER code, in fp64"""
    cb = torch.from_numpy(np.array(cb, dtype=np.float64))
    rows = torch.as_tensor(np.asarray(rows), dtype=torch.int64)
    if cb.shape[0] == 1:
        return np.zeros(rows.shape[0], dtype=np.int64)
    out = []
    for lo in range(0, rows.shape[0], 1024):
        r = rows[lo:lo + 1024]
        a = cb[r]
        d = sum((a[:, None, i] - cb[None, :, i]) ** 2 for i in range(3))
        d[torch.arange(r.shape[0]), r] = float("inf")
        out.append(d.argmin(1))
    return torch.cat(out).numpy()


def random(n, k, seed=0):
    r = _rng("random", k, seed)          # not keyed by n: the first m tokens of the family at n are the family at m
    return (r.randn(n, 3) * 1.3).astype(np.float32), codebook(k, 0.7, False, seed)


def midpoint(n, k, scale=0.7, shifted=False, seed=0):
    """every token the fp32-rounded midpoint of a random code and that code's nearest neighbour: two distances that differ by roundings"""
    cb = codebook(k, scale, shifted, seed)
    j = _rng("mid", k, scale, shifted, seed).randint(0, k, size=n)
    used, inv = np.unique(j, return_inverse=True)
    nn = nearest_neighbour(cb, used)[inv]
    z = ((cb[j].astype(np.float64) + cb[nn].astype(np.float64)) / 2).astype(np.float32)
    return z, cb


def duplicate_pairs(k):
    """(lower, upper) rows that hold the same code: row j and row j + k // 2 -- in different ranges for 16, 8 and 4 parts -- and, where there is
    more than one resident chunk, a row of chunk 0 and the last row (K = 16 385: j and j + 8192 are the first kind, (1, 16 384) the second)"""
    h = k // 2
    if h == 0:
        return []
    js = sorted(set(np.linspace(0, h - 1, min(h, 48)).astype(int).tolist()))
    pairs = [(j, j + h) for j in js]
    if k > CHUNK and (k - 1) not in [u for _, u in pairs]:
        free = [j for j in range(min(h, 16)) if j not in js] or [None]
        if free[0] is not None:
            pairs.append((free[0], k - 1))
    return pairs


def duplicate(n, k, seed=0):
    """tokens EQUAL to duplicated rows: both copies give the same distance bits, the lower index must win"""
    cb = codebook(k, 0.7, False, seed).copy()
    pairs = duplicate_pairs(k)
    for lo, hi in pairs:
        cb[hi] = cb[lo]
    if not pairs:
        return random(n, k, seed)[0], cb, np.zeros(0, dtype=np.int64)
    lower = np.asarray([lo for lo, _ in pairs], dtype=np.int64)
    pick = np.arange(n) % len(pairs)
    pick = _rng("dup", k, seed).permutation(len(pairs))[pick]
    return cb[[pairs[p][1] for p in pick]].copy(), cb, lower[pick]          # built from the UPPER copy: the same bits


def special_plants(n):
    """{position: kind} inside a run of n tokens: a NaN token at 0, and for EVERY listed count m <= n a token holding +inf at m - 1, a NaN
    token at m // 2 and one holding -inf at m // 3 -- so that the first m tokens of the family are the family at m tokens"""
    plants = {}
    for m in sorted(SMALL_N + LARGE_N + (n,)):
        if 3 < m <= n:
            plants[m // 3] = "-inf"
            plants[m // 2] = "nan"
            plants[m - 1] = "+inf"
    plants[0] = "nan"
    return plants


def special(n, k, seed=0):
    """random tokens with special_plants(n); NaN rows in the codebook at K // 2 and (one component) K - 1 when K >= 4, so that a finite row
    always exists"""
    z, cb = random(n, k, seed + 1)
    z, cb = z.copy(), cb.copy()
    if k >= 4:
        cb[k // 2] = np.nan
        cb[k - 1, 1] = np.nan
    for p, kind in special_plants(n).items():
        if kind == "nan":
            z[p] = np.nan
        elif kind == "+inf":
            z[p, 2] = np.inf
        else:
            z[p, 0] = -np.inf
    return z, cb


def family(name, n, k, seed=0):
    """-> (tokens fp32 [n, 3], codebook fp32 [k, 3])"""
    if name == "random":
        return random(n, k, seed)
    if name == "midpoint0.7":
        return midpoint(n, k, 0.7, False, seed)
    if name == "midpoint30":
        return midpoint(n, k, 30.0, False, seed)
    if name == "midpoint_shifted":
        return midpoint(n, k, 0.7, True, seed)
    if name == "duplicate":
        return duplicate(n, k, seed)[:2]
    if name == "special":
        return special(n, k, seed)
    raise KeyError(name)


# ---- the oracle, over the host's threads -------------------------------------------------------------------------------------------------
def oracle(z, cb, threads=16):
    """oracle.c_ref.vq_nearest on slices of the tokens (tokens are independent; ctypes releases the GIL)"""
    from oracle import c_ref

    n = z.shape[0]
    if n < 4096:
        return c_ref.vq_nearest(z, cb)
    c_ref.lib()
    cuts = np.linspace(0, n, threads + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda i: c_ref.vq_nearest(z[cuts[i]:cuts[i + 1]], cb), range(threads)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


# ---- the fp64 check ----------------------------------------------------------------------------------------------------------------------
def excess(z, cb, idx, device="cpu", step=2048):
    """-> (per token (d64(chosen) - min d64) / (C_ROUND U ((zz + ee_chosen) + (zz + ee_best))), the fp64 argmin); tokens that hold a NaN or an
    infinity give 0 (the special family pins those to the oracle), a codebook row that holds one is at distance +inf"""
    z, cb, idx = (torch.from_numpy(np.array(a)) if isinstance(a, np.ndarray) else a for a in (z, cb, idx))
    z, cb, idx = z.to(device).double(), cb.to(device).double(), idx.to(device)
    ee = (cb * cb).sum(1)
    bad_row = ~torch.isfinite(ee)
    ratio, best = [], []
    for lo in range(0, z.shape[0], step):
        a, i = z[lo:lo + step], idx[lo:lo + step]
        d = sum((a[:, None, c] - cb[None, :, c]) ** 2 for c in range(3))
        d = torch.where(bad_row[None, :], torch.full_like(d, float("inf")), d)
        dmin, amin = d.min(1)
        zz = (a * a).sum(1)
        dch = d.gather(1, i[:, None])[:, 0]
        r = (dch - dmin) / (C_ROUND * U * ((zz + ee[i]) + (zz + ee[amin])))
        ok = torch.isfinite(zz)
        ratio.append(torch.where(ok, r, torch.zeros_like(r)))
        best.append(amin)
    return torch.cat(ratio), torch.cat(best)


# ---- the kernel's search in fp32, with its structure and its mutations -------------------------------------------------------------------
MUTATIONS = ("last_range_skipped", "merge_keeps_higher_index", "fma_in_zz")


def _r32(x):
    return x.astype(np.float32).astype(np.float64)


def distances_f32(z, cb, mutation=None):
    """[n, K] the kernel's d, every rounding spelled: fp32 operands in fp64, rounded to fp32 after each operation (a product of two fp32
    numbers is exact in fp64; an fma's sum rounds once to 53 bits, then to 24 -- the same as one rounding unless the 53-bit sum ends in a tie)"""
    z, cb = z.astype(np.float64), cb.astype(np.float64)
    with np.errstate(all="ignore"):
        if mutation == "fma_in_zz":
            zz = _r32(z[:, 2] * z[:, 2] + _r32(z[:, 1] * z[:, 1] + _r32(z[:, 0] * z[:, 0])))
        else:
            zz = _r32(_r32(_r32(z[:, 0] * z[:, 0]) + _r32(z[:, 1] * z[:, 1])) + _r32(z[:, 2] * z[:, 2]))
        ee = _r32(_r32(_r32(cb[:, 0] * cb[:, 0]) + _r32(cb[:, 1] * cb[:, 1])) + _r32(cb[:, 2] * cb[:, 2]))
        dot = _r32(z[:, None, 0] * cb[None, :, 0])
        dot = _r32(z[:, None, 1] * cb[None, :, 1] + dot)
        dot = _r32(z[:, None, 2] * cb[None, :, 2] + dot)
        return _r32(_r32(zz[:, None] + ee[None, :]) - 2.0 * dot)


def search_f32(z, cb, n_tokens_of_launch=None, mutation=None):
    """the kernel's choice: per (chunk, part) the first minimum, then the merge by (distance, index); no distance below +inf -> 0.
    n_tokens_of_launch picks the number of parts (default: the number of tokens given)."""
    n, k = z.shape[0], cb.shape[0]
    parts = parts_for(n if n_tokens_of_launch is None else n_tokens_of_launch)
    d = distances_f32(z, cb, mutation)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isnan(d), np.inf, d)          # `d < best` is false for a NaN: it is never taken
    best = np.full((parts, n), np.inf)
    bidx = np.full((parts, n), 0x7fffffff, dtype=np.int64)
    for c0 in range(0, k, CHUNK):
        nc = min(CHUNK, k - c0)
        rs = ranges(nc, parts)
        for p, (lo, hi) in enumerate(rs):
            if hi <= lo or (mutation == "last_range_skipped" and p == parts - 1):
                continue
            blk = d[:, c0 + lo:c0 + hi]
            a = blk.argmin(1)                         # the first minimum
            v = blk[np.arange(n), a]
            take = v < best[p]
            best[p] = np.where(take, v, best[p])
            bidx[p] = np.where(take, c0 + lo + a, bidx[p])
    b, i = best[0].copy(), bidx[0].copy()
    for p in range(1, parts):
        if mutation == "merge_keeps_higher_index":
            take = (best[p] < b) | ((best[p] == b) & (bidx[p] > i) & (bidx[p] != 0x7fffffff))
        else:
            take = (best[p] < b) | ((best[p] == b) & (bidx[p] < i))
        b, i = np.where(take, best[p], b), np.where(take, bidx[p], i)
    return np.where(i == 0x7fffffff, 0, i)
