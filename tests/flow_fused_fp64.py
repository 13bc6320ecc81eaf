"""One fused coupling step of the flow's reverse pass (csrc/flow_fused.hip, glare_flow_step_fused_bf16) restated in plain fp64 torch from the
fp32 operands the C ABI receives: the reference of test_gpu_flow_fused_edges.py, checked on the CPU against oracle.torch_ref.FlowStep, its
exact family proven representable and every comparison shown sensitive (test_flow_fused_fp64_host.py).  A plain module like tolerances.py;
nothing here touches the library, the 16-bit format is an argument.

    h1 = relu(ftA[.., a_off : a_off + 64] + conv3x3(z_in[.., 0], wz, zero pad))
    h2 = relu(W2 h1 + b2)                       (then zero outside the image)
    h4 = b4 + conv3x3(h2, W4, zero pad)
    z1 = z1 / (sigmoid(h4[1] + 2) + eps) - h4[0];   z2 = z2 / (sigmoid(h4[3] + 2) + eps) - h4[2]
    z0, z1, z2 = z_k / (sigmoid(f[2k + 1] + 2) + eps) - f[2k],   f = hF[.., f_off : f_off + 6]
    z_out = M z + t

The restatement works on the REGION grid, (H + 2) x (W + 2) pixels, region pixel (ry, rx) = image pixel (ry - 1, rx - 1): h1 and h2 exist on
the one-pixel ring around the image too, computed from a clamped ftA pixel and the zero-padded z0 as the kernel computes them, and are then
zeroed there -- so that "not zeroed" is a mutation that can be written down.  The 3x3 conv 64 -> 4 is the kernel's 36 rows S[tap 4 + cout]
per region pixel and a 9-tap shift-add.

BOUND of the random family (step_fp64; U = 2^-24, one fp32 rounding), counted from flow_fused.hip, per element:
  every MFMA product (_product: fs_split8 + fs_mfma3), on x' = the fp32 value the kernel splits, |x' - x| <= ex, and the fp32 filter w:
    input     ex through |w|
    x pair    x' = hi + lo + r, |r| <= conv_fp64.pair_slack(x, ex) (lo rounds once), through |w_hi| + |w_lo|
    w pair    w = w_hi + w_lo + rw, rw known exactly, times |x| + ex
    dropped   the kernel contracts w_hi x_hi + w_lo x_hi + w_hi x_lo: sum |w_lo| |x_lo|, |x_lo| <= 0.5 ulp16(|x| + ex)
    MFMA      conv_fp64.mfma_slack(3 K, mag): THREE products per k-step chained on one accumulator, K = 16 (9 taps, 7 zero), 64, 64;
              mag = (|w_hi| + |w_lo|) (|x_hi| + |x_lo|) + |initial accumulator| (ftA, b2, 0)
  relu        1-Lipschitz, and an exact 0 on both sides where the exact value lies below minus its own bound; the zeroing outside the image is
              exact (the packed registers are set to 0)
  shift-add   h = b4, then 9 fp32 additions of S rows: the rows' own errors, and 9 U (|b4| + sum |S| + their errors)
  tail        flow.hip's flow_tail in the same op order; _scale64 / _unscale64 / _affine64 are test_gpu_streaming_edges.py's counts, restated here
              with the errors h4 brings: on the shift directly, on the scale's argument a through sigmoid'(a) ea + 0.05 ea^2 (|sigmoid''| <
              0.1), relative to s; eps is a parameter
  chained     a second step takes the first step's bound as `ez`: on z0 through |wz| (the `input` term of the first product) and on z0, z1, z2
              through the tail
EXACT FAMILY (exact_operands): every value the kernel forms up to h4 is exact (exact_report asserts it: pairs exact, dropped sums zero,
every sum of magnitudes below 2^24 of its unit), so h4 is the fp64 h4 and the bound on z_out is flow_tail's alone (h4_exact=True).
  "int"      z0 non-zero integers in [-2, 2], wz integers in [-2, 2], ftA integers in [-4, 4], W2 +-1 at density 0.25, b2 integers in [-3, 3],
             W4 +-2^-9 at density 0.5, b4 multiples of 1/4 in [-3/4, 3/4]: every lo is zero
  "act_lo"   ftA and b2 multiples of 2^-8: h1 and h2 carry a lo (|h2| < 256: 16 bits, a bf16 pair)
  "wz_lo"    wz = +-(1 + 2^-9) under bf16, +-(1 + 2^-11) under fp16: the FILTER carries a lo in either format (1 + 2^-9 is a number of fp16);
             h1 and h2 carry one too, W2 and W4 have none, so nothing is dropped
  "w2_lo"    W2 = +-(1 + that bit): the second product's filter carries the lo, h1 (integers) has none, h2 acquires one, W4 has none
  "w4_lo"    W4 = +-2^-9 (1 + that bit): the third product's filter carries the lo, h1 and h2 are integers
             -- so a w_lo . x_hi product that is dropped or paired with the wrong fragment is a unit error of h4 in EACH of the three products
z1, z2, hF, M, t are ordinary fp32 normals; every image of a batch is drawn on its own, so a read from the wrong image is a unit error."""
import torch
import torch.nn.functional as F

import conv_fp64 as C
from conv_fp64 import U

TH, TW = 16, 40          # interior pixels of a workgroup's tile (FsGeom<16, 40, 8>)
FORMATS = (torch.bfloat16, torch.float16)
FLOW_EPS = 1e-4
# (B, H, W): every halo pixel outside; a one-pixel axis with a second tile of one column / row; exactly one tile (block 23's padding lanes
# live); 2 x 2 tiles with seams; 3 x 3 tiles, one with its whole halo inside the image
SIZES = ((3, 1, 1), (2, 1, 41), (2, 17, 1), (1, 16, 40), (2, 17, 41), (3, 33, 81))
EXACT_VARIANTS = ("int", "act_lo", "wz_lo", "w2_lo", "w4_lo")
FAMILIES = EXACT_VARIANTS + ("random",)
A_LAYOUTS = ((192, 64), (68, 4))          # (pitch, offset) of ftA; 68 / 4 is the tightest the ABI admits with a non-zero offset
F_LAYOUTS = ((16, 8), (8, 0), (12, 4))

MUTATIONS = ("wz_taps_transposed", "h2_not_zeroed", "z0_clamped", "halo_from_previous_image", "w2_channels_exchanged", "w4_tap_cout_exchanged",
             "b2_omitted", "b4_omitted", "eps_omitted", "h4_01_exchanged", "hF_one_float_off", "M_transposed", "wlo_xhi_dropped", "whi_xlo_dropped")
DROPPED = ("wlo_xhi_dropped", "whi_xlo_dropped")


def f32(v):
    """a Python number as the C `float` argument the ABI receives, back as a double"""
    return float(torch.tensor(v, dtype=torch.float32))


def lo_bit(dtype):
    """1 + this is hi = 1 with a non-zero lo in `dtype` (1 + 2^-9 is a number of fp16)"""
    return 2.0 ** -9 if dtype == torch.bfloat16 else 2.0 ** -11


def units(variant, dtype):
    """the exact family's granularity: (h1, h2, S / h4) are whole multiples of these"""
    k = lo_bit(dtype)
    return {"int": (1.0, 1.0, 2.0 ** -9), "act_lo": (2.0 ** -8, 2.0 ** -8, 2.0 ** -17), "wz_lo": (k, k, k * 2.0 ** -9), "w2_lo": (1.0, k, k * 2.0 ** -9),
            "w4_lo": (1.0, 1.0, k * 2.0 ** -9)}[variant]


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
def _tail_operands(g, B, H, W):
    return dict(hF=torch.randn(B, H, W, 8, generator=g), M=torch.randn(3, 3, generator=g), t=torch.randn(3, generator=g))


def exact_operands(B, H, W, variant="int", dtype=torch.bfloat16, seed=0, eps=FLOW_EPS):
    """-> dict of fp32 CPU tensors: z [B, H, W, 3], ftA [B, H, W, 64] (the window), wz [64, 9], w2 [64, 64], b2 [64], w4 [4, 64, 3, 3], b4 [4],
    hF [B, H, W, 8] (floats 0 .. 5 are the window, 6 and 7 what a read one float off would see), M [3, 3], t [3], eps"""
    g = torch.Generator().manual_seed(4242 + 1000 * H + 10 * W + B + 7919 * seed + EXACT_VARIANTS.index(variant))

    def ints(lo, hi, shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    def signs(shape):
        return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()

    z = torch.randn(B, H, W, 3, generator=g) * 0.7
    z[..., 0] = signs((B, H, W)) * ints(1, 2, (B, H, W))
    wz = ints(-2, 2, (64, 9))
    ftA = ints(-4, 4, (B, H, W, 64))
    w2 = signs((64, 64)) * (torch.rand(64, 64, generator=g) < 0.25).float()
    b2 = ints(-3, 3, (64,))
    w4 = signs((4, 64, 3, 3)) * (torch.rand(4, 64, 3, 3, generator=g) < 0.5).float() * 2.0 ** -9
    b4 = ints(-3, 3, (4,)) / 4.0
    if variant == "act_lo":
        ftA = ints(-4 * 256, 4 * 256, (B, H, W, 64)) / 256.0
        b2 = ints(-3 * 256, 3 * 256, (64,)) / 256.0
    elif variant == "wz_lo":
        wz = signs((64, 9)) * (1.0 + lo_bit(dtype))
    elif variant == "w2_lo":
        w2 = w2 * (1.0 + lo_bit(dtype))
    elif variant == "w4_lo":
        w4 = w4 * (1.0 + lo_bit(dtype))
    else:
        assert variant == "int", variant
    return dict(z=z, ftA=ftA, wz=wz, w2=w2, b2=b2, w4=w4, b4=b4, eps=f32(eps), family=variant, **_tail_operands(g, B, H, W))


def random_operands(B, H, W, seed=0, eps=FLOW_EPS):
    """plain fp32 normals: z ~ N(0, 0.7), ftA ~ N(0, 1), wz ~ 0.1 N, W2 ~ N / 8, W4 ~ N / 24 (h1^2 ~ 1/2, h2^2 ~ 1/4: h4 has a standard deviation
    near 0.5), b2 ~ 0.3 N, b4 ~ 0.3 N -- filters and z0 all need their lo"""
    g = torch.Generator().manual_seed(99 + 1000 * H + 10 * W + B + 7919 * seed)
    return dict(z=torch.randn(B, H, W, 3, generator=g) * 0.7, ftA=torch.randn(B, H, W, 64, generator=g), wz=torch.randn(64, 9, generator=g) * 0.1,
                w2=torch.randn(64, 64, generator=g) / 8.0, b2=torch.randn(64, generator=g) * 0.3, w4=torch.randn(4, 64, 3, 3, generator=g) / 24.0,
                b4=torch.randn(4, generator=g) * 0.3, eps=f32(eps), family="random", **_tail_operands(g, B, H, W))


def operands(B, H, W, family, dtype, seed=0, eps=FLOW_EPS):
    return random_operands(B, H, W, seed, eps) if family == "random" else exact_operands(B, H, W, family, dtype, seed, eps)


# ---- the pieces of the step ---------------------------------------------------------------------------------------------------------------
def _pair(v, dtype):
    hi, lo = C.pair16(v, dtype)
    return hi.double(), lo.double()


def _product(x, ex, w, init, K, dtype, drop=None):
    """x [.., C] fp64 (exact), ex its error bound, w [Co, C] the fp32 filter as fp64, init the accumulator's initial value ([.., Co] or [Co])
    -> (w x + init, bound of the kernel's fp32 accumulator against it): the five terms of the module's header.  drop: a mutation's missing product"""
    wh, wl = _pair(w, dtype)
    val = x @ w.t() + init
    if drop is not None:
        xh, xl = _pair(x, dtype)
        val = val - (xh @ wl.t() if drop == "wlo_xhi_dropped" else xl @ wh.t())
    rw, wa = (w - wh - wl).abs(), wh.abs() + wl.abs()
    xb = x.abs() + ex
    half = 0.5 * C.ulp16(xb, dtype)          # |x_lo|, and |x' - x_hi|
    mag = (xb + 2.0 * half) @ wa.t() + init.abs()
    err = ex @ w.abs().t() + C.pair_slack(x, ex, dtype) @ wa.t() + xb @ rw.t() + half @ wl.abs().t() + C.mfma_slack(3 * K, mag)
    return val, err


def _relu(v, e):
    """relu is 1-Lipschitz; where the exact value lies below -e the kernel's own value is negative too and its relu is the same exact 0"""
    return v.clamp_min(0.0), torch.where(v < -e, torch.zeros_like(e), e)


def _scale64(x, ex, eps):
    """s = sigmoid(x + 2) + eps in fp64 and the RELATIVE error bound of the kernel's s: its fp32 evaluation 1 / (1 + expf(-(x + 2))) + eps --
    a = x + 2 rounds once, which moves e = expf(-a) by |a| U relative; expf itself 2 ulp = 4 U; 1 + e rounds once and damps e's error by
    e / (1 + e) = 1 - sigmoid; the division 1 U; + eps rounds once: ((1 - sig) (4 + |a|) + 3) U, taken at the worst argument within ex --
    on top of the argument's own error: sigmoid'(a) ex + 0.05 ex^2"""
    a = x + 2.0
    sig = torch.sigmoid(a)
    s = sig + eps
    rs = (torch.sigmoid(-(a - ex)) * (4.0 + a.abs() + ex) + 3.0) * U
    ds = (sig * (1.0 - sig) * ex + 0.05 * ex * ex) / s
    return s, ds + rs * (1.0 + ds)


def _unscale64(z, ez, x_scale, e_scale, shift, e_shift, eps):
    """z / s - shift: z's error over s, s's relative error on |q| (both over 1 - rel: it is 1 / s' the kernel multiplies into), the division
    (1 U), the shift's error, the subtraction (1 U)"""
    s, rel = _scale64(x_scale, e_scale, eps)
    q = z / s
    eq = (ez / s + q.abs() * rel) / (1.0 - rel)
    eq = eq + U * (q.abs() + eq)
    return q - shift, eq + e_shift + U * (q.abs() + eq + shift.abs() + e_shift)


def _affine64(v, ev, M, t):
    """M v + t as three chained fmas per row: the input errors through |M|, 3 roundings on the magnitudes of the terms"""
    out = v @ M.t() + t
    mag = (v.abs() + ev) @ M.abs().t() + t.abs()
    return out, ev @ M.abs().t() + 3 * U * mag


def region(o, mutate=None, ez=None):
    """-> the operands on the region grid: patches [B, H + 2, W + 2, 9] of z0 (tap t = 3 ky + kx reads image pixel (y + ky - 1, x + kx - 1), zero
    outside the image), their error bound, ftA of the CLAMPED pixel [B, H + 2, W + 2, 64], inside [H + 2, W + 2]"""
    z = o["z"].double()
    B, H, W, _ = z.shape
    z0 = z[..., 0].unsqueeze(1)
    z0p = F.pad(z0, (2, 2, 2, 2), mode="replicate") if mutate == "z0_clamped" else F.pad(z0, (2, 2, 2, 2))
    e0p = F.pad((torch.zeros_like(z) if ez is None else ez)[..., 0].unsqueeze(1), (2, 2, 2, 2))
    taps = [(t // 3, t % 3) for t in range(9)]
    patches = torch.stack([z0p[:, 0, ky:ky + H + 2, kx:kx + W + 2] for ky, kx in taps], -1)
    epatches = torch.stack([e0p[:, 0, ky:ky + H + 2, kx:kx + W + 2] for ky, kx in taps], -1)
    iy, ix = (torch.arange(H + 2) - 1).clamp(0, H - 1), (torch.arange(W + 2) - 1).clamp(0, W - 1)
    a = o["ftA"].double()[:, iy][:, :, ix]
    inside = torch.zeros(H + 2, W + 2, dtype=torch.float64)
    inside[1:H + 1, 1:W + 1] = 1.0
    return patches, epatches, a, inside


def filters(o, mutate=None):
    """-> wz [64, 9], W2 [64, 64], b2, W4 as the kernel's 36 rows [tap 4 + cout, 64], b4 (fp64), with a mutation's change"""
    wz, w2, b2, w4, b4 = (o[n].double() for n in ("wz", "w2", "b2", "w4", "b4"))
    if mutate == "wz_taps_transposed":
        wz = wz.view(64, 3, 3).transpose(1, 2).reshape(64, 9)
    if mutate == "w2_channels_exchanged":          # input channels 0 and 1: elements i = 0, 1 of k-step (j, u) = (0, 0), half 0
        w2 = w2.clone()
        w2[:, [0, 1]] = w2[:, [1, 0]]
    w4r = w4.permute(2, 3, 0, 1).reshape(36, 64)
    if mutate == "w4_tap_cout_exchanged":          # packed as row = cout 9 + tap, read as tap 4 + cout
        w4r = w4.reshape(4, 64, 9).permute(0, 2, 1).reshape(36, 64)
    if mutate == "b2_omitted":
        b2 = torch.zeros_like(b2)
    if mutate == "b4_omitted":
        b4 = torch.zeros_like(b4)
    return wz, w2.reshape(64, 64), b2, w4r, b4


def hidden(o, dtype, mutate=None, ez=None):
    """-> dict: h1, h2 (region grid, exact), S [B, H + 2, W + 2, 9, 4], h4 [B, H, W, 4] and the error bounds e1, e2, eS, e4"""
    B, H, W, _ = o["z"].shape
    patches, epatches, a, inside = region(o, mutate, ez)
    wz, w2, b2, w4r, b4 = filters(o, mutate)
    drop = mutate if mutate in DROPPED else None
    h1, e1 = _relu(*_product(patches, epatches, wz, a, 16, dtype, drop))
    h2, e2 = _relu(*_product(h1, e1, w2, b2, 64, dtype, drop))
    keep = torch.ones_like(inside) if mutate == "h2_not_zeroed" else inside
    h2, e2 = h2 * keep.view(1, H + 2, W + 2, 1), e2 * keep.view(1, H + 2, W + 2, 1)
    S, eS = _product(h2, e2, w4r, torch.zeros(36, dtype=torch.float64), 64, dtype, drop)
    eS = eS * keep.view(1, H + 2, W + 2, 1)          # zeroed registers contract to an exact 0
    S, eS = S.view(B, H + 2, W + 2, 9, 4), eS.view(B, H + 2, W + 2, 9, 4)
    Sp = S.roll(1, 0)
    ty, tx = torch.arange(H).view(H, 1) // TH, torch.arange(W).view(1, W) // TW
    h4 = b4.expand(B, H, W, 4).clone()
    smag, es = b4.abs().expand(B, H, W, 4).clone(), torch.zeros(B, H, W, 4, dtype=torch.float64)
    for t in range(9):
        ky, kx = t // 3, t % 3
        s = S[:, ky:ky + H, kx:kx + W, t]
        if mutate == "halo_from_previous_image":          # a tap that reads ANOTHER tile's pixel (inside the image) reads it in image b - 1
            ny, nx = torch.arange(H).view(H, 1) + ky - 1, torch.arange(W).view(1, W) + kx - 1
            other = ((ny >= 0) & (ny < H) & (nx >= 0) & (nx < W) & ((ny // TH != ty) | (nx // TW != tx))).view(1, H, W, 1)
            s = torch.where(other, Sp[:, ky:ky + H, kx:kx + W, t], s)
        h4 = h4 + s
        smag = smag + s.abs() + eS[:, ky:ky + H, kx:kx + W, t]
        es = es + eS[:, ky:ky + H, kx:kx + W, t]
    return dict(h1=h1, e1=e1, h2=h2, e2=e2, S=S, eS=eS, h4=h4, e4=es + 9 * U * smag)


def step_fp64(o, dtype, mutate=None, ez=None, h4_exact=None):
    """-> (z_out [B, H, W, 3] fp64, its per-element bound, the hidden values).  ez: the error bound of z_in (a chained step).  h4_exact: the
    exact family's bound, h4 without error (default: the operands' own family decides)"""
    z = o["z"].double()
    ez = torch.zeros_like(z) if ez is None else ez
    hid = hidden(o, dtype, mutate, ez)
    h4, e4 = hid["h4"], hid["e4"]
    if (o["family"] != "random") if h4_exact is None else h4_exact:
        e4 = torch.zeros_like(e4)
    eps = 0.0 if mutate == "eps_omitted" else float(o["eps"])
    if mutate == "h4_01_exchanged":
        h4, e4 = h4[..., [1, 0, 2, 3]], e4[..., [1, 0, 2, 3]]
    f = o["hF"].double()[..., 1:7] if mutate == "hF_one_float_off" else o["hF"].double()[..., 0:6]
    zero = torch.zeros_like(z[..., 0])
    v1, e1 = _unscale64(z[..., 1], ez[..., 1], h4[..., 1], e4[..., 1], h4[..., 0], e4[..., 0], eps)
    v2, e2 = _unscale64(z[..., 2], ez[..., 2], h4[..., 3], e4[..., 3], h4[..., 2], e4[..., 2], eps)
    v = [_unscale64(z[..., 0], ez[..., 0], f[..., 1], zero, f[..., 0], zero, eps), _unscale64(v1, e1, f[..., 3], zero, f[..., 2], zero, eps),
         _unscale64(v2, e2, f[..., 5], zero, f[..., 4], zero, eps)]
    M = o["M"].double().t() if mutate == "M_transposed" else o["M"].double()
    out, bound = _affine64(torch.stack([a for a, _ in v], -1), torch.stack([e for _, e in v], -1), M, o["t"].double())
    return out, bound, hid


# ---- the exact family's rule, as code -----------------------------------------------------------------------------------------------------
def exact_report(o, dtype):
    """What makes the exact family exact, measured on one set of operands in one format -> dict:
      pairs     the largest |v - hi - lo| over z0, the three filters, h1 and h2 (must be 0)
      dropped   the largest dropped sum |w_lo| |x_lo| of the three contractions, conv_fp64.split3's third result (must be 0)
      replay    the largest difference between split3's three-product contraction and the fp64 value (must be 0)
      units     the largest magnitude sum of each contraction -- and of the shift-add -- in its own unit (must stay below 2^24), and whether every
                value is a whole multiple of that unit
      lo        how many lo halves are non-zero in the filters and in the activations"""
    B, H, W, _ = o["z"].shape
    patches, _, a, inside = region(o)
    wz, w2, b2, w4r, b4 = filters(o)
    hid = hidden(o, dtype)
    u1, u2, u3 = units(o["family"], dtype)
    rep = dict(pairs=0.0, dropped=0.0, replay=0.0, whole=True, mags=[], lo_w=0, lo_x=0)
    stages = ((patches, wz, a, hid["h1"], u1, True), (hid["h1"], w2, b2, hid["h2"], u2, True), (hid["h2"], w4r, None, hid["S"].reshape(B, H + 2, W + 2, 36), u3, False))
    for x, w, init, want, unit, relu in stages:
        xh, xl = _pair(x, dtype)
        wh, wl = _pair(w, dtype)
        rep["pairs"] = max(rep["pairs"], float((x - xh - xl).abs().max()), float((w - wh - wl).abs().max()))
        rep["lo_w"] += int((wl != 0).sum())
        rep["lo_x"] += int((xl != 0).sum())
        acc, mag, dropped = C.split3(xh, xl, w.reshape(w.shape[0], w.shape[1], 1, 1), dtype)
        if init is not None:
            acc, mag = acc + init, mag + init.abs()
        if relu:
            acc = acc.clamp_min(0.0)
            if want is hid["h2"]:
                acc = acc * inside.view(1, H + 2, W + 2, 1)
        rep["dropped"] = max(rep["dropped"], float(dropped.max()))
        rep["replay"] = max(rep["replay"], float((acc - want).abs().max()))
        rep["mags"].append(float(mag.max()) / unit)
        rep["whole"] = rep["whole"] and bool(torch.equal(want / unit, (want / unit).round())) and bool(torch.equal(mag / unit, (mag / unit).round()))
    smag = b4.abs().expand(B, H, W, 4).clone()
    for t in range(9):
        smag = smag + hid["S"][:, t // 3:t // 3 + H, t % 3:t % 3 + W, t].abs()
    rep["mags"].append(float(smag.max()) / u3)
    rep["whole"] = rep["whole"] and bool(torch.equal(hid["h4"] / u3, (hid["h4"] / u3).round()))
    return rep, hid
