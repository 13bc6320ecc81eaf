"""The forward convolutions restated in plain fp64 torch: the references of test_gpu_conv_edges.py.  Written from the contract in
include/glare_hip.h (glare_conv_desc, glare_conv2d_smallcin_f32, glare_conv1x1_ws_*) with explicit index arithmetic on an explicitly
padded image -- not from the kernels -- and checked on the CPU against F.conv2d, F.interpolate, F.pad and fp64 autograd
(test_conv_fp64_host.py), which also shows that the comparisons SEE one removed tap product, a halo column shifted by one, a halo row
taken from the next image, the bias of the neighbouring channel and a dropped K tail.  Nothing here touches the library; the 16-bit
format is an argument.

Every function returns, per output element, the exact value and `mag` = sum |terms| (the same conv on |x|, |w|): the bound of the
GPU file is counted on it.

ROUNDING POINTS, as the kernels document them (read in csrc/conv_igemm_kernel.h, csrc/conv1x1.hip, csrc/conv_small.hip):
    LDS-staged 16-bit epilogue (EPI_FAST, every kernel family) and the plain weight-stationary 1x1 kernel:
        t = round16(act?(acc + bias))      the activation here only when there is NO residual (none / relu; sigmoid / swish without a
                                           residual never take this epilogue: conv_pick_epilogue)
        out = round16(act(t + residual))   with a residual: TWO roundings (staged16)
    general epilogue (EPI_GENERAL: odd Cout / pitch / offset, fp32 NHWC, 16-bit planes, sigmoid / swish on the accumulators) and the
    planar fp32 epilogue (EPI_PLANAR):
        out = round(act(acc + bias + residual))      nothing rounded before the residual add: ONE rounding (none for fp32)
    hi / lo epilogue (HILO instantiations of the implicit-GEMM kernel, glare_conv1x1_ws_hilo_bf16, glare_conv1x1_ws_split_bf16,
    glare_conv2d_smallcin_hilo_f32):
        v = act(acc + bias + residual_hi + residual_lo) in fp32, hi = round16(v), lo = round16(v - hi)   (pair16; v - hi is exact in fp32)
    conv_small: an fp32 FMA chain that STARTS at the bias (k k cin roundings), then the activation, then one rounding of the output.
The sub-pixel filters are the 3x3 taps that read one source pixel summed in fp32 and rounded ONCE (subpixel_filters); with
feedback=True the four phase filters are rounded by the sequential error-feedback definition instead (feedback_round)."""
import torch

U = 2.0 ** -24            # one fp32 rounding, relative

# ---- geometry and dispatch, restated from csrc/conv_igemm.hip (pick_variant, glare_conv2d_bf16) and conv_igemm_kernel.h --------------
TILE_ROWS, TILE_COLS = 8, 32          # WM * MT == 8 in every instantiation the launchers name (no 6-wave 12 x 32 variant is instantiated)
NHWC16, NHWC32, PLANAR32, PLANAR16 = 0, 1, 2, 3          # GLARE_OUT_*; test_capi.py pins the header's values


def out_size(H, W, ksize, stride, upsample):
    IH, IW = (2 * H, 2 * W) if upsample else (H, W)
    if stride == 2:
        return (IH + 1 - 3) // 2 + 1, (IW + 1 - 3) // 2 + 1
    return IH, IW


def pick_tile(ksize, cout, cout_tile=0):
    """-> (output-channel tile, channels per K stage)"""
    tn = 128 if cout > 64 else (64 if cout > 32 else 32)
    if cout_tile in (32, 64) and cout_tile < tn:
        tn = cout_tile
    return tn, (32 if ksize == 1 else 16)


def padded_k(ksize, cin_total, subpixel=False):
    """products per output element the implicit-GEMM kernel multiplies: whole K stages (zero-filled beyond Cin) x taps"""
    kc = 32 if ksize == 1 else 16
    taps = 4 if subpixel else ksize * ksize
    return -(-cin_total // kc) * kc * taps


def igemm_dispatch(ksize, stride, subpixel, cout, cout_tile, out_mode, out_pitch, out_off, res, res_pitch, res_off, act, hilo=False, gnp=False):
    """-> (kernel family, tile, epilogue) of a launch glare_conv2d_bf16 accepts"""
    tn, _ = pick_tile(ksize, cout, cout_tile)
    family = "k2" if subpixel else ("k1" if ksize == 1 else ("k3s2" if stride == 2 else "k3s1"))
    fast = out_mode == NHWC16 and cout % 8 == 0 and out_pitch % 8 == 0 and out_off % 8 == 0 and (not res or (res_pitch % 8 == 0 and res_off % 8 == 0))
    expk = act in ("sigmoid", "swish")
    if hilo:
        assert fast and not subpixel
        return family, tn, "hilo"
    if fast and not (not res and expk):
        epi = "fast"
    elif family == "k3s1" and out_mode == PLANAR32 and not res and not expk:
        epi = "planar"
    else:
        epi = "general"
    if gnp:
        assert family == "k3s1" and tn == 128 and epi == "fast"
        epi = "gnp"
    return family, tn, epi


def ws_supported(cin, cout, split=False):
    ct = 64 if split else 128
    return cin in (128, 256, 512) and cout > 0 and cout % ct == 0 and cout // ct <= 32 and 32 % (cout // ct) == 0


# ---- the operator ----------------------------------------------------------------------------------------------------------------------
def act64(v, act):
    if act == "relu":
        return v.clamp_min(0.0)
    if act == "sigmoid":
        return torch.sigmoid(v)
    if act == "swish":
        return v * torch.sigmoid(v)
    assert act == "none", act
    return v


def window(buf, off, c):
    """channels [off, off + c) of a [..., pitch] buffer as fp64"""
    assert 0 <= off and off + c <= buf.shape[-1]
    return buf[..., off:off + c].double()


def padded_input(x, upsample):
    """x [B, H, W, C] -> the conv's input with ONE ring of zeros around it, [B, IH + 2, IW + 2, C]: the nearest x2 upsample repeats every
    source pixel twice along both axes; pixel (iy, ix) of the conv's input is element (iy + 1, ix + 1)."""
    if upsample:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    B, IH, IW, C = x.shape
    xp = torch.zeros(B, IH + 2, IW + 2, C, dtype=x.dtype, device=x.device)
    xp[:, 1:IH + 1, 1:IW + 1] = x
    return xp


def conv_taps(xp, w, stride, OH, OW):
    """xp from padded_input, w [Co, C, k, k] -> [B, OH, OW, Co]: out[b, oy, ox, co] = sum_{ty, tx, c} in[b, oy s + ty - pad, ox s + tx - pad, c]
    w[co, c, ty, tx], pad = k // 2 under stride 1, 0 under stride 2 (whose (0,1,0,1) padding is the zero ring's far side)."""
    k = w.shape[2]
    pad = k // 2 if stride == 1 else 0
    oy = torch.arange(OH, device=xp.device) * stride - pad + 1
    ox = torch.arange(OW, device=xp.device) * stride - pad + 1
    out = torch.zeros(xp.shape[0], OH, OW, w.shape[0], dtype=xp.dtype, device=xp.device)
    for ty in range(k):
        for tx in range(k):
            out += torch.einsum("bhwc,oc->bhwo", xp[:, oy + ty][:, :, ox + tx], w[:, :, ty, tx])
    return out


def conv_acc(x, w, stride=1, upsample=False):
    OH, OW = out_size(x.shape[1], x.shape[2], w.shape[2], stride, upsample)
    return conv_taps(padded_input(x, upsample), w, stride, OH, OW)


class Ref:
    """acc = sum of the products, mag = sum of their magnitudes, bias [Co] and res [B, OH, OW, Co] (zeros when absent), all fp64"""

    def __init__(self, acc, mag, bias, res, has_res):
        self.acc, self.mag, self.bias, self.res, self.has_res = acc, mag, bias, res, has_res

    def pre(self):
        return self.acc + self.bias + self.res

    def value(self, act="none"):
        return act64(self.pre(), act)

    def mag_all(self):
        return self.mag + self.bias.abs() + self.res.abs()


def conv_front(x_buf, w, bias=None, *, cin=None, in_off=0, x2_buf=None, cin2=None, in2_off=0, stride=1, upsample=False,
               residual_buf=None, res_off=0):
    """The conv front end of glare_conv_desc on whole buffers: channels [in_off, in_off + cin) of x_buf [B, H, W, pitch], an optional second
    source concatenated behind them, w fp64 [Co, cin + cin2, k, k], residual channels [res_off, res_off + Co) of its own buffer."""
    cin = x_buf.shape[-1] - in_off if cin is None else cin
    x = window(x_buf, in_off, cin)
    if x2_buf is not None:
        cin2 = x2_buf.shape[-1] - in2_off if cin2 is None else cin2
        x = torch.cat([x, window(x2_buf, in2_off, cin2)], -1)
    assert w.shape[1] == x.shape[-1] and w.shape[2] in (1, 3) and (stride == 1 or w.shape[2] == 3)
    acc, mag = conv_acc(x, w, stride, upsample), conv_acc(x.abs(), w.abs(), stride, upsample)
    co = w.shape[0]
    b = torch.zeros(co, dtype=torch.float64, device=acc.device) if bias is None else bias.double()
    r = torch.zeros_like(acc) if residual_buf is None else window(residual_buf, res_off, co)
    assert r.shape == acc.shape, (r.shape, acc.shape)
    return Ref(acc, mag, b, r, residual_buf is not None)


def staged16(ref, act, dtype):
    """the LDS-staged epilogue's two roundings, as fp64 values of `dtype` numbers"""
    if not ref.has_res:
        return act64(ref.acc + ref.bias, act).to(dtype).double()
    t = (ref.acc + ref.bias).to(dtype).double()
    return act64(t + ref.res, act).to(dtype).double()


def pair16(v, dtype):
    """hi = round16(v), lo = round16(v - hi)"""
    hi = v.to(dtype)
    return hi, (v - hi.double()).to(dtype)


def place(buf, values, out_mode, out_off):
    """`values` [B, OH, OW, Co] written into a copy of the sentinel-filled `buf` as the output mode lays it out: NHWC [B, OH, OW, pitch] at
    channel out_off; planar [B, planes, plane_pitch] at plane out_off, pixel oy OW + ox, the [OH OW, plane_pitch) tail of a plane not written"""
    e = buf.clone()
    B, OH, OW, Co = values.shape
    v = values.to(buf.dtype)
    if out_mode in (NHWC16, NHWC32):
        e[..., out_off:out_off + Co] = v
    else:
        e[:, out_off:out_off + Co, :OH * OW] = v.permute(0, 3, 1, 2).reshape(B, Co, OH * OW)
    return e


def owned(buf, shape, out_mode, out_off):
    """the inverse of place(): the launch's own elements of `buf` as [B, OH, OW, Co]"""
    B, OH, OW, Co = shape
    if out_mode in (NHWC16, NHWC32):
        return buf[..., out_off:out_off + Co]
    return buf[:, out_off:out_off + Co, :OH * OW].reshape(B, Co, OH, OW).permute(0, 2, 3, 1)


# ---- the sub-pixel form of "nearest x2 upsample, then 3x3" -----------------------------------------------------------------------------
SUBPIXEL_TAPS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}          # output parity a -> the 3x3 rows (columns alike) behind source offset r = 0, 1


def subpixel_filters(w, dtype=None):
    """w [Co, C, 3, 3] -> [4, Co, C, 2, 2], phase 2 a + b: the taps that read one source pixel summed (ky-major, kx-minor, from 0, in fp32 when
    `dtype` is given, then rounded once to it)."""
    acc_t = torch.float64 if dtype is None else torch.float32
    ph = torch.zeros(4, w.shape[0], w.shape[1], 2, 2, dtype=acc_t, device=w.device)
    for a in (0, 1):
        for b in (0, 1):
            for r in (0, 1):
                for c in (0, 1):
                    for ky in SUBPIXEL_TAPS[a][r]:
                        for kx in SUBPIXEL_TAPS[b][c]:
                            ph[2 * a + b, :, :, r, c] = ph[2 * a + b, :, :, r, c] + w[:, :, ky, kx].to(acc_t)
    return ph.double() if dtype is None else ph.to(dtype).double()


def feedback_round(w, dtype):
    """glare_filter_feedback_round_bf16's definition: along the flattened trailing axes of every leading index, q_i = round16(float(w_i +
    carry)), carry = (w_i + carry) - q_i in double."""
    flat = w.double().reshape(w.shape[0], -1)
    out = torch.empty_like(flat)
    carry = torch.zeros(flat.shape[0], dtype=torch.float64, device=w.device)
    for i in range(flat.shape[1]):
        t = flat[:, i] + carry
        q = t.float().to(dtype).double()
        out[:, i] = q
        carry = t - q
    return out.reshape(w.shape)


def subpixel_conv(x, ph):
    """x [B, H, W, C], ph [4, Co, C, 2, 2] -> [B, 2 H, 2 W, Co]: out[b, 2 i + a, 2 j + b'] = sum_{r, c} x[b, i - 1 + a + r, j - 1 + b' + c]
    ph[2 a + b', :, :, r, c], 0 outside the source"""
    B, H, W, C = x.shape
    xp = padded_input(x, False)
    out = torch.zeros(B, 2 * H, 2 * W, ph.shape[1], dtype=x.dtype, device=x.device)
    for a in (0, 1):
        for b in (0, 1):
            for r in (0, 1):
                for c in (0, 1):
                    out[:, a::2, b::2] += torch.einsum("bhwc,oc->bhwo", xp[:, a + r:a + r + H, b + c:b + c + W], ph[2 * a + b, :, :, r, c])
    return out


# ---- the data-gradient pack ------------------------------------------------------------------------------------------------------------
def dgrad_filter(w, pad_to):
    """forward filter [Co, Ci, k, k] -> the filter [Ci, pad_to, k, k] of the stride-1 conv that maps dL/dy (Co channels, zero-padded to pad_to)
    to dL/dx: w'[ci, co, tap] = w[co, ci, k k - 1 - tap], zero for co >= Co"""
    Co, Ci, k, _ = w.shape
    out = torch.zeros(Ci, pad_to, k, k, dtype=w.dtype, device=w.device)
    out[:, :Co] = w.flip(2, 3).transpose(0, 1)
    return out


# ---- conv2d_smallcin -------------------------------------------------------------------------------------------------------------------
def strided_nhwc(x_flat, strides, B, H, W, C):
    """the [B, H, W, C] tensor that element strides (sb, sc, sy, sx) address in a flat buffer"""
    sb, sc, sy, sx = strides
    idx = (torch.arange(B).view(B, 1, 1, 1) * sb + torch.arange(H).view(1, H, 1, 1) * sy + torch.arange(W).view(1, 1, W, 1) * sx
           + torch.arange(C).view(1, 1, 1, C) * sc).to(x_flat.device)
    return x_flat.reshape(-1)[idx]


def smallcin(x_flat, strides, B, H, W, w, bias=None):
    x = strided_nhwc(x_flat, strides, B, H, W, w.shape[1]).double()
    acc, mag = conv_acc(x, w), conv_acc(x.abs(), w.abs())
    b = torch.zeros(w.shape[0], dtype=torch.float64, device=acc.device) if bias is None else bias.double()
    return Ref(acc, mag, b, torch.zeros_like(acc), False)


# ---- the fp32-class form ---------------------------------------------------------------------------------------------------------------
def split3(x_hi, x_lo, w, dtype, stride=1):
    """pair activation [B, H, W, C] (fp64 values of 16-bit numbers), fp32 filter w as fp64 -> (what the kernel contracts: x_hi w_hi + x_lo w_hi
    + x_hi w_lo, the magnitudes of those products, the DROPPED sum |x_lo| |w_lo|), w_hi = round16(w), w_lo = round16(w - w_hi)"""
    w_hi = w.float().to(dtype).double()
    w_lo = (w.float() - w_hi.float()).to(dtype).double()
    acc = conv_acc(x_hi, w_hi, stride) + conv_acc(x_lo, w_hi, stride) + conv_acc(x_hi, w_lo, stride)
    mag = conv_acc(x_hi.abs(), w_hi.abs(), stride) + conv_acc(x_lo.abs(), w_hi.abs(), stride) + conv_acc(x_hi.abs(), w_lo.abs(), stride)
    return acc, mag, conv_acc(x_lo.abs(), w_lo.abs(), stride)


# ---- fused GroupNorm statistics --------------------------------------------------------------------------------------------------------
def gn_stats(y):
    """y [B, OH, OW, C] fp64 -> ([B, 1, 32, 2] sum and sum of squares per (image, group of C / 32 adjacent channels), the same of |y|, y^2:
    equal for the second moment)"""
    B, OH, OW, C = y.shape
    g = y.reshape(B, OH * OW, 32, C // 32)
    return torch.stack([g.sum(dim=(1, 3)), (g * g).sum(dim=(1, 3))], -1).unsqueeze(1), torch.stack([g.abs().sum(dim=(1, 3)), (g * g).sum(dim=(1, 3))], -1).unsqueeze(1)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------
def fmt(dtype):
    return (7, -126) if dtype == torch.bfloat16 else (10, -14)


def ulp16(v, dtype):
    m, emin = fmt(dtype)
    v = v.double().abs().clamp_min(2.0 ** emin)
    e = torch.floor(torch.log2(v))
    e = torch.where(torch.exp2(e) > v, e - 1, e)
    e = torch.where(torch.exp2(e + 1) <= v, e + 1, e)
    return torch.exp2(e.clamp_min(emin) - m)


def mfma_slack(kp, mag):
    """a sum of kp products on the MFMA: 2 U (kp + 1) sum |terms| (test_gpu_disc_kernels.py states the rule)"""
    return 2.0 * U * (kp + 1) * mag


def binade_extra(exact, slack, dtype):
    """what 0.5 ulp16(exact) + slack misses when the value the kernel rounds lies within `slack` ABOVE the next power of two"""
    return 0.5 * (ulp16(exact.abs() + slack, dtype) - ulp16(exact, dtype))


def pair_slack(exact, slack, dtype):
    """the rounding of lo = round16(v - hi): |v - hi| <= 0.5 ulp16(v), so half an ulp16 of that (2^-22-class in fp16, 2^-16-class in bf16;
    the format's subnormal spacing where lo is that small)"""
    return 0.5 * ulp16(0.5 * ulp16(exact.abs() + slack, dtype), dtype)


def sigmoid_rel(a, arg_roundings=2):
    """test_gpu_backward_edges._sigmoid_rel (its docstring has the count): relative error of 1 / (1 + __expf(-a)) in fp32"""
    return (torch.sigmoid(-a) * (4.0 + arg_roundings * a.abs()) + 2.0) * U


def act_slack(v, e_v, act):
    """error of act(v) evaluated in fp32 on an argument within e_v of v.  none / relu: 1-Lipschitz, exact.  sigmoid = 1 / (1 + __expf(-v)),
    swish = v / (1 + __expf(-v)): the same relative error (the numerator is exact) on top of |f'| e_v, f'' <= 1/2 on the way there."""
    if act in ("none", "relu"):
        return e_v
    s = torch.sigmoid(v)
    if act == "sigmoid":
        return (s * (1 - s) + 0.5 * e_v) * e_v + s * sigmoid_rel(v)
    return ((s + v * s * (1 - s)).abs() + 0.5 * e_v) * e_v + (v * s).abs() * sigmoid_rel(v)


# ---- operand generators ----------------------------------------------------------------------------------------------------------------
LIMIT = {torch.bfloat16: 2.0 ** 8, torch.float16: 2.0 ** 11, torch.float32: 2.0 ** 24}          # integers every format holds exactly up to here


def _signs(gen, shape):
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).double()


def int_density(K, x_second_moment=1.0):
    """fraction of non-zero filter taps (+-1) that keeps 8 standard deviations of a sum of K products below 200 < 2^8 - |bias| - |residual|;
    never below 0.54: no operand tensor is zero in half of its elements"""
    return max(0.54, min(1.0, 625.0 / (K * x_second_moment)))


def int_operands(gen, x_shape, w_shape):
    """x: +-1 everywhere (K > 64) or non-zero integers in [-2, 2]; w: +-1 at density int_density(K) (K <= 64: non-zero in [-2, 2])"""
    K = w_shape[1] * w_shape[2] * w_shape[3]
    if K <= 64:
        x = _signs(gen, x_shape) * torch.randint(1, 3, x_shape, generator=gen).double()
        w = _signs(gen, w_shape) * torch.randint(1, 3, w_shape, generator=gen).double()
    else:
        x = _signs(gen, x_shape)
        w = _signs(gen, w_shape) * (torch.rand(w_shape, generator=gen) < int_density(K)).double()
    return x, w


def int_bias(gen, co):
    return torch.randint(-3, 4, (co,), generator=gen).double()


def int_residual(gen, shape):
    return _signs(gen, shape) * torch.randint(1, 5, shape, generator=gen).double()


def normal_operands(gen, x_shape, w_shape, dtype):
    """N(0, 1) activations with |x| >= 2^-6 and N(0, 1 / K) filters with |w| >= 2^-10, both rounded to `dtype`: normal-range 16-bit numbers
    in either format, so every MFMA product is exact in fp32"""
    K = w_shape[1] * w_shape[2] * w_shape[3]
    x = torch.randn(x_shape, generator=gen)
    w = torch.randn(w_shape, generator=gen) / K ** 0.5
    x = torch.where(x < 0, -1.0, 1.0) * x.abs().clamp_min(2.0 ** -6)
    w = torch.where(w < 0, -1.0, 1.0) * w.abs().clamp_min(2.0 ** -10)
    return x.to(dtype).double(), w.to(dtype).double()


def normal16(gen, shape, dtype, scale=1.0):
    x = torch.randn(shape, generator=gen) * scale
    return (torch.where(x < 0, -1.0, 1.0) * x.abs().clamp_min(2.0 ** -6)).to(dtype).double()


# ---- the cases of the implicit-GEMM kernel: shared by the GPU file (which launches them) and the host file (which checks the restatement and
# the operand conditions on each).  geometry: (B, H, W, ksize, stride, upsample), channels: (cin, cin2, cout), cout_tile, out_mode, flags
def case(name, B, H, W, k, stride, ups, cin, cin2, cout, tile=0, mode=NHWC16, res=False, act="none", bias=True, odd_pitch=False,
         subpixel=False, stats=False, want=None):
    return dict(name=name, B=B, H=H, W=W, k=k, stride=stride, ups=ups, cin=cin, cin2=cin2, cout=cout, tile=tile, mode=mode, res=res, act=act,
                bias=bias, odd_pitch=odd_pitch, subpixel=subpixel, stats=stats, want=want)


IGEMM_CASES = [
    # 3x3 stride 1, LDS-staged epilogue: every tile width, ragged and exact tile edges, the K tail, two sources, the upsample
    case("k3s1 128 ragged", 2, 9, 33, 3, 1, False, 24, 0, 128, act="relu", want=("k3s1", 128, "fast")),
    case("k3s1 128 res stats", 2, 17, 65, 3, 1, False, 16, 0, 128, res=True, stats=True, want=("k3s1", 128, "fast")),
    case("k3s1 136 K=1152", 1, 9, 32, 3, 1, False, 128, 0, 136, res=True, act="relu", want=("k3s1", 128, "fast")),
    case("k3s1 72 tile 64", 2, 8, 32, 3, 1, False, 40, 0, 72, tile=64, want=("k3s1", 64, "fast")),
    case("k3s1 40 tile 32", 2, 7, 31, 3, 1, False, 72, 0, 40, tile=32, res=True, want=("k3s1", 32, "fast")),
    case("k3s1 8 one pixel", 2, 1, 1, 3, 1, False, 8, 0, 8, want=("k3s1", 32, "fast")),
    case("k3s1 256 two sources", 2, 8, 33, 3, 1, False, 16, 32, 256, act="relu", want=("k3s1", 128, "fast")),
    case("k3s1 64 upsample of 1x1", 2, 1, 1, 3, 1, True, 32, 0, 64, want=("k3s1", 64, "fast")),
    case("k3s1 32 upsample", 2, 5, 17, 3, 1, True, 16, 0, 32, res=True, want=("k3s1", 32, "fast")),
    # 3x3 stride 1, general epilogue
    case("k3s1 general cout 3", 2, 17, 33, 3, 1, False, 16, 0, 3, want=("k3s1", 32, "general")),
    case("k3s1 general pitch 20", 2, 9, 31, 3, 1, False, 8, 0, 8, odd_pitch=True, res=True, act="relu", want=("k3s1", 32, "general")),
    case("k3s1 general fp32 res", 2, 8, 31, 3, 1, False, 24, 0, 72, mode=NHWC32, res=True, act="relu", want=("k3s1", 128, "general")),
    case("k3s1 general 16-bit planes", 2, 7, 9, 3, 1, False, 16, 0, 64, mode=PLANAR16, want=("k3s1", 64, "general")),
    case("k3s1 general sigmoid", 2, 9, 33, 3, 1, False, 16, 0, 32, act="sigmoid", want=("k3s1", 32, "general")),
    case("k3s1 general swish fp32", 1, 8, 32, 3, 1, False, 32, 0, 136, mode=NHWC32, act="swish", want=("k3s1", 128, "general")),
    # 3x3 stride 1, planar fp32 epilogue (conv_offset: 108 planes, padded)
    case("k3s1 planar 108", 2, 9, 33, 3, 1, False, 32, 0, 108, mode=PLANAR32, want=("k3s1", 128, "planar")),
    case("k3s1 planar 40 tile 32", 1, 17, 31, 3, 1, False, 16, 0, 40, tile=32, mode=PLANAR32, act="relu", want=("k3s1", 32, "planar")),
    # 3x3 stride 2: odd and even sides, 2 x 2 -> 1 x 1
    case("k3s2 128 odd", 2, 9, 33, 3, 2, False, 16, 0, 128, act="relu", want=("k3s2", 128, "fast")),
    case("k3s2 64 even res", 2, 8, 66, 3, 2, False, 24, 0, 64, res=True, want=("k3s2", 64, "fast")),
    case("k3s2 32 2x2", 2, 2, 2, 3, 2, False, 32, 0, 32, want=("k3s2", 32, "fast")),
    case("k3s2 general fp32", 2, 17, 65, 3, 2, False, 16, 16, 3, mode=NHWC32, want=("k3s2", 32, "general")),
    # 1x1 on the implicit-GEMM kernel (shapes the weight-stationary kernel does not take)
    case("k1 72 K tail", 2, 9, 33, 1, 1, False, 40, 0, 72, res=True, act="relu", want=("k1", 128, "fast")),
    case("k1 256 two sources", 2, 8, 31, 1, 1, False, 32, 64, 256, want=("k1", 128, "fast")),
    case("k1 40 tile 32", 2, 1, 31, 1, 1, False, 8, 0, 40, tile=32, want=("k1", 32, "fast")),
    case("k1 general fp32 136", 2, 1, 33, 1, 1, False, 72, 0, 136, mode=NHWC32, res=True, want=("k1", 128, "general")),
    case("k1 general V^T planes", 2, 5, 7, 1, 1, False, 128, 0, 128, mode=PLANAR16, want=("k1", 128, "general")),
    # the sub-pixel form
    case("k2 64 of 1x1", 2, 1, 1, 3, 1, True, 16, 0, 64, subpixel=True, want=("k2", 64, "fast")),
    case("k2 128 res stats", 2, 9, 33, 3, 1, True, 32, 0, 128, subpixel=True, res=True, stats=True, want=("k2", 128, "fast")),
    case("k2 40 K tail", 1, 8, 32, 3, 1, True, 24, 0, 40, subpixel=True, act="relu", want=("k2", 64, "fast")),
]


def case_layout(c):
    """-> the channel windows of a case: every operand a window of a wider buffer (offsets multiples of 8, pitch > off + channels) unless the
    fused statistics need the output to own its tensor; odd_pitch: an output of pitch 20 at offset 4"""
    lay = dict(in_pitch=c["cin"] + 24, in_off=8, in2_pitch=c["cin2"] + 16, in2_off=8, res_pitch=c["cout"] + 16 if c["cout"] % 8 == 0 else c["cout"] + 5,
               res_off=8 if c["cout"] % 8 == 0 else 2)
    OH, OW = out_size(c["H"], c["W"], c["k"], c["stride"], c["ups"])
    if c["mode"] in (PLANAR32, PLANAR16):
        lay.update(out_pitch=c["cout"] + 4, out_off=2, plane_pitch=-(-OH * OW // 32) * 32 + 32)
    elif c["stats"]:
        lay.update(out_pitch=c["cout"], out_off=0, plane_pitch=0)
    elif c["odd_pitch"]:
        lay.update(out_pitch=20, out_off=4, plane_pitch=0, res_pitch=20, res_off=4)
    elif c["cout"] % 8:
        lay.update(out_pitch=c["cout"] + 6, out_off=2, plane_pitch=0)
    else:
        lay.update(out_pitch=c["cout"] + 16, out_off=8, plane_pitch=0)
    return lay


def case_dispatch(c):
    lay = case_layout(c)
    return igemm_dispatch(c["k"], c["stride"], c["subpixel"], c["cout"], c["tile"], c["mode"], lay["out_pitch"], lay["out_off"], c["res"],
                          lay["res_pitch"], lay["res_off"], c["act"])


def case_operands(c, family, dtype):
    """-> dict of fp64 CPU tensors: x [B, H, W, cin], x2 or None, w [cout, cin + cin2, k, k], bias or None, res [B, OH, OW, cout] or None.
    family "int": the exact-arithmetic operands; "normal": 16-bit normal operands of `dtype`."""
    gen = torch.Generator().manual_seed(sum(ord(ch) for ch in c["name"]) * 7 + (family == "int"))
    B, H, W, k, ct = c["B"], c["H"], c["W"], c["k"], c["cin"] + c["cin2"]
    OH, OW = out_size(H, W, k, c["stride"], c["ups"])
    if family == "int":
        x, w = int_operands(gen, (B, H, W, ct), (c["cout"], ct, k, k))
        bias = int_bias(gen, c["cout"]) if c["bias"] else None
        res = int_residual(gen, (B, OH, OW, c["cout"])) if c["res"] else None
    else:
        x, w = normal_operands(gen, (B, H, W, ct), (c["cout"], ct, k, k), dtype)
        bias = torch.randn(c["cout"], generator=gen).float().double() * 0.25 if c["bias"] else None
        res = normal16(gen, (B, OH, OW, c["cout"]), dtype) if c["res"] else None
    return dict(x=x[..., :c["cin"]].contiguous(), x2=x[..., c["cin"]:].contiguous() if c["cin2"] else None, w=w, bias=bias, res=res)


def case_reference(c, ops_, dtype=None):
    """the restatement on a case's operands (already windows) -> Ref; the sub-pixel form contracts subpixel_filters(w, dtype)"""
    x = ops_["x"] if ops_["x2"] is None else torch.cat([ops_["x"], ops_["x2"]], -1)
    w = ops_["w"]
    if c["subpixel"]:
        ph = subpixel_filters(w, dtype)
        acc, mag = subpixel_conv(x, ph), subpixel_conv(x.abs(), ph.abs())
    else:
        acc, mag = conv_acc(x, w, c["stride"], c["ups"]), conv_acc(x.abs(), w.abs(), c["stride"], c["ups"])
    b = torch.zeros(c["cout"], dtype=torch.float64, device=acc.device) if ops_["bias"] is None else ops_["bias"].to(acc.device)
    r = torch.zeros_like(acc) if ops_["res"] is None else ops_["res"].to(acc.device)
    return Ref(acc, mag, b, r, ops_["res"] is not None)


def case_bound(c, ref, dtype):
    """-> (exact, slack) of a case's BOUNDED comparison: 2 U (Kp + 1) sum |terms| for the MFMA chain, 2 U |.| per epilogue addition (bias,
    residual), the staged epilogue's intermediate rounding where it applies, the activation's own evaluation; the caller adds the
    output's 0.5 ulp16 (assert_rounded) unless the output is fp32."""
    family, _, epi = c["want"]
    kp = padded_k(c["k"], c["cin"] + c["cin2"], c["subpixel"])
    mag = ref.mag_all()
    e = mfma_slack(kp, ref.mag) + 2.0 * U * mag * (1 if c["bias"] else 0)
    if epi == "fast" and c["res"]:
        t = ref.acc + ref.bias
        e = e + 0.5 * ulp16(t.abs() + e, dtype)          # round16(acc + bias), before the residual add
    if c["res"]:
        e = e + 2.0 * U * mag
    return ref.value(c["act"]), act_slack(ref.pre(), e, c["act"])
