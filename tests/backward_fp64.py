"""The adjoints of the streaming kernels restated in plain torch, for fp64 operands: the references of test_gpu_backward_edges.py.
Each is written from the mathematics in the header comments of csrc/flow_bwd.hip and csrc/train_ops.hip (the forward operation and
its derivative), not from the kernels' loops, and test_backward_fp64_host.py checks every one against fp64 AUTOGRAD of the forward
operation -- so that the GPU test's reference is not a copy of the code under test.  Tensors keep the kernels' layouts (channels
last); where a kernel leaves per-block partial sums, the restatement returns the per-pixel TERMS of the sum and the test adds
them over the pixels it expects a block to own.  The second half holds the references of test_gpu_matrix_backward.py: attention on
base-2 logits and its backward (the header of csrc/attn_bwd.hip), the row softmax, the weight gradient of csrc/wgrad.hip, and the
exact-arithmetic operands of the fused backward with their single-term condition.  A plain module like tolerances.py."""
import torch
import torch.nn.functional as F

TAPS = [(t // 3 - 1, t % 3 - 1) for t in range(9)]          # tap t of a 3x3 filter reads the pixel at offset (dy, dx)


def per_sample(v, like):
    """[B] -> [B, 1, ...] broadcastable against `like` ([B, ...])"""
    return v.reshape([-1] + [1] * (like.dim() - 1))


# ---- Gaussian log-density: logp[b] = sum -0.5 ((z - mean)^2 + log 2 pi) ----------------------------------------------------------
def nll_backward(z, mean, g_logp):
    """-> (gz, gmean): d logp / d mean = z - mean, d logp / d z = -(z - mean), times the sample's g_logp"""
    g = per_sample(g_logp, z) * (z - mean)
    return -g, g


# ---- affine coupling: scale = sigmoid(raw + 2) + eps ------------------------------------------------------------------------------
def coupling_scale(raw, eps):
    sg = torch.sigmoid(raw + 2.0)
    return sg, sg + eps


def _coupling_adjoint(g, pre, shift, raw, gl, eps):
    """out = (pre + shift) * scale and logdet += log scale  ->  (g_pre = g_shift, g_raw):
    d out / d pre = d out / d shift = scale;  d / d raw = (g (pre + shift) + gl / scale) scale'(raw), scale' = sg (1 - sg)"""
    sg, s = coupling_scale(raw, eps)
    return g * s, (g * (pre + shift) + gl / s) * sg * (1.0 - sg)


def post_backward(gz, z_pre, h4, g_logdet, eps):
    """z''[0] = z'[0]; z''[1 + c] = (z'[1 + c] + h4[2c]) * scale(h4[2c + 1]); logdet[b] += sum log scale.
    gz, z_pre [B, ..., 3]; h4 [B, ..., 4] -> (gz' [B, ..., 3], gh4 [B, ..., 4])"""
    gl = per_sample(g_logdet, gz[..., 0])
    cols, gh = [gz[..., 0]], []
    for c in range(2):
        gp, gr = _coupling_adjoint(gz[..., 1 + c], z_pre[..., 1 + c], h4[..., 2 * c], h4[..., 2 * c + 1], gl, eps)
        cols.append(gp)
        gh += [gp, gr]
    return torch.stack(cols, -1), torch.stack(gh, -1)


def pre_backward(gz, z_in, f6, g_logdet, M, t, eps):
    """y = M z + t; z'[i] = (y[i] + f6[2i]) * scale(f6[2i + 1]); logdet[b] += sum log scale.
    -> (gz_in = M^T gy, gf6 [B, ..., 6], gy [B, ..., 3]); gM = sum over pixels of gy (x) z, gt = sum of gy: see pre_terms"""
    gl = per_sample(g_logdet, gz[..., 0])
    y = z_in @ M.t() + t
    gy, gf = [], []
    for i in range(3):
        gp, gr = _coupling_adjoint(gz[..., i], y[..., i], f6[..., 2 * i], f6[..., 2 * i + 1], gl, eps)
        gy.append(gp)
        gf += [gp, gr]
    gy = torch.stack(gy, -1)
    return gy @ M, torch.stack(gf, -1), gy


def pre_terms(gy, z_in):
    """per-pixel terms of (gM row-major, gt): [B, ..., 12]"""
    return torch.cat([(gy.unsqueeze(-1) * z_in.unsqueeze(-2)).flatten(-2), gy], -1)


# ---- h1 = conv3x3(z0 -> 64 channels, pad 1) ---------------------------------------------------------------------------------------
def _shifted(img, dy, dx):
    """[B, H, W, ...] -> the image read at offset (dy, dx): out[y, x] = img[y + dy, x + dx], zero outside"""
    B, H, W = img.shape[:3]
    out = torch.zeros_like(img)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    yd, xd = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    out[:, ys, xs] = img[:, yd, xd]
    return out


def h1_backward_data(g, wz):
    """g [B, H, W, 64], wz [64, 9] -> the gradient of z0 [B, H, W]: z0[p] fed h1[p - d_t] through tap t"""
    return sum(_shifted(g, -dy, -dx) @ wz[:, t] for t, (dy, dx) in enumerate(TAPS))


def h1_filter_terms(g, z0):
    """per-pixel terms of the filter gradient [B, H, W, 64, 9]: h1[p] saw z0[p + d_t] through tap t"""
    zt = torch.stack([_shifted(z0, dy, dx) for dy, dx in TAPS], -1)
    return g.unsqueeze(-1) * zt.unsqueeze(-2)


# ---- GroupNorm(32) [+ swish] ------------------------------------------------------------------------------------------------------
def swish_grad(u):
    s = torch.sigmoid(u)
    return s * (1.0 + u * (1.0 - s))


def groupnorm_backward(x, dy, gamma, beta, mean, rstd, swish):
    """x, dy [B, HW, C]; mean, rstd [B, 32] (of the group's HW * C / 32 values).  u = xh gamma + beta, xh = (x - mean) rstd,
    y = swish(u) or u.  du = dy swish'(u);  s1 = sum_p du, s2 = sum_p du xh  (dbeta, dgamma = their sums over the images);
    dx = rstd (du gamma - mean_group(du gamma) - xh mean_group(du gamma xh))  -> (dx, s1 [B, C], s2 [B, C], xh, du)"""
    B, HW, C = x.shape
    cpg = C // 32
    mu, r = (v.repeat_interleave(cpg, 1).unsqueeze(1) for v in (mean, rstd))
    xh = (x - mu) * r
    du = dy * swish_grad(xh * gamma + beta) if swish else dy
    s1, s2 = du.sum(1), (du * xh).sum(1)
    m = float(HW * cpg)
    a = ((s1 * gamma).view(B, 32, cpg).sum(2) / m).repeat_interleave(cpg, 1).unsqueeze(1)
    q = ((s2 * gamma).view(B, 32, cpg).sum(2) / m).repeat_interleave(cpg, 1).unsqueeze(1)
    return r * (du * gamma - a - xh * q), s1, s2, xh, du


# ---- mix: out = s a + (1 - s) b, s = sigmoid(w) -----------------------------------------------------------------------------------
def mix_backward(g, a, b, w):
    """-> (ga, gb, dw): d out / d w = (a - b) s (1 - s)"""
    s = torch.sigmoid(w)
    return s * g, (1.0 - s) * g, s * (1.0 - s) * (g * (a - b)).sum()


# ---- mean rescale: out = h + xw r, r = sum h / sum xw over the sample (or over the batch) -------------------------------------
def mean_rescale_sums(g, h, xw, whole):
    """[B, n] -> (D = sum g xw, Sh, Sx), each [B] (the batch's totals repeated when `whole`)"""
    D, Sh, Sx = (g * xw).sum(1), h.sum(1), xw.sum(1)
    if whole:
        D, Sh, Sx = (v.sum().expand(g.shape[0]) for v in (D, Sh, Sx))
    return D, Sh, Sx


def mean_rescale_backward(g, h, xw, whole):
    """d out_j / d h_i = delta_ij + xw_j / Sx;  d out_j / d xw_i = delta_ij r - xw_j Sh / Sx^2
    -> (gh = g + D / Sx, gxw = g r - D Sh / Sx^2)"""
    D, Sh, Sx = (v.unsqueeze(1) for v in mean_rescale_sums(g, h, xw, whole))
    return g + D / Sx, g * (Sh / Sx) - D * Sh / (Sx * Sx)


# ---- activations the forward convs fuse: the derivative in terms of the OUTPUT y --------------------------------------------------
def act_backward(g, y, act):
    if act == "relu":
        return torch.where(y > 0, g, torch.zeros_like(g))
    assert act == "sigmoid"
    return g * y * (1.0 - y)


# ---- the forward operations (for autograd; test_backward_fp64_host.py) ------------------------------------------------------------
def h1_forward(z0, wz):
    """z0 [B, H, W], wz [64, 9] -> [B, H, W, 64]"""
    return F.conv2d(z0.unsqueeze(1), wz.view(64, 1, 3, 3), padding=1).permute(0, 2, 3, 1)


# ---- single-head attention on base-2 logits (csrc/attn.hip, csrc/attn_bwd.hip) -----------------------------------------------------
def attention_fp64(q, k, v):
    """q (scale and log2 e folded in), k, v [B, N, d] -> (O [B, N, d], L [B, N]): s_ij = q_i . k_j, L_i = log2 sum_j 2^s_ij,
    O_i = sum_j 2^(s_ij - L_i) v_j"""
    s = q @ k.transpose(-1, -2)
    m = s.amax(-1, keepdim=True)
    e = torch.exp2(s - m)
    l = e.sum(-1, keepdim=True)
    return (e / l) @ v, (m + torch.log2(l)).squeeze(-1)


def attention_backward_terms(q, k, v, o, do, L, ln2_scale):
    """-> (s, p, dp, D, ds): p = 2^(s - L), dp = do . v, D = do . o, ds = ln2_scale p (dp - D).  `o` and `L` are INPUTS, as they are
    for the kernel (the header of csrc/attn_bwd.hip): nothing here recomputes them"""
    s = q @ k.transpose(-1, -2)
    p = torch.exp2(s - L.unsqueeze(-1))
    dp = do @ v.transpose(-1, -2)
    D = (do * o).sum(-1)
    return s, p, dp, D, ln2_scale * p * (dp - D.unsqueeze(-1))


def attention_backward_fp64(q, k, v, o, do, L, ln2_scale):
    """-> (dq = ds k, dk = ds^T q, dv = p^T do, D)"""
    _, p, _, D, ds = attention_backward_terms(q, k, v, o, do, L, ln2_scale)
    return ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do, D


def softmax2_rows_fp64(S):
    """P_ij = 2^S_ij / sum_j 2^S_ij"""
    e = torch.exp2(S - S.amax(-1, keepdim=True))
    return e / e.sum(-1, keepdim=True)


def attention_ds_fp64(P, dP, dO, O, scale):
    """dS_ij = scale P_ij (dP_ij - delta_i), delta_i = dO_i . O_i -> (dS, delta)"""
    delta = (dO * O).sum(-1)
    return scale * P * (dP - delta.unsqueeze(-1)), delta


# ---- weight gradient of a k x k / stride-1 / pad k // 2 convolution (csrc/wgrad.hip) ------------------------------------------------
def conv_weight_grad_fp64(x, g, ksize):
    """x [B, H, W, Ci], g [B, H, W, Co] -> (dW [Co, Ci, k, k], db [Co]): dW[co][ci][ty][tx] = sum_{b,y,x} g[b][y][x][co]
    x[b][y + ty - h][x + tx - h][ci] with zeros outside the image (h = k // 2), db[co] = sum g"""
    h = ksize // 2
    taps = [torch.einsum("byxo,byxi->oi", g, _shifted(x, ty - h, tx - h)) for ty in range(ksize) for tx in range(ksize)]
    return torch.stack(taps, -1).view(g.shape[-1], x.shape[-1], ksize, ksize), g.sum((0, 1, 2))


# ---- exact-arithmetic operands of the fused attention backward (test_gpu_matrix_backward.py, section 5) ---------------------------
EXACT_CH = (0, 300)          # the two score channels, one in each 256-channel half
# (B, N) of the fused backward's per-element tests: one token; 1 / 1 / 2 streamed tiles of 32 with the 64-row resident block mostly empty;
# the resident block boundary and an image offset with a ragged tail; 4 tiles, 2 blocks; 5 tiles (odd) and 9 workgroups (XCD remap
# remainder 1); 12 workgroups (remainder 4); the size of test_gpu_train.py
ATTN_CASES = ((1, 1), (1, 31), (1, 32), (1, 33), (2, 63), (1, 64), (2, 65), (1, 97), (3, 129), (3, 200), (1, 330))
EXACT_CASES = ATTN_CASES + ((2, 1000),)          # 32 tiles, the split-key forward's size
EXACT_CASE_LARGE = (1, 105 * 155)                # one 400 x 600 image's latent, 16 275 tokens: run on the GPU only (2.6e8 scores)
FORMATS = {"bf16": (7, -126), "fp16": (10, -14)}          # mantissa bits, smallest normal exponent


def exact_attention_case(B, N):
    """Operands with which every product, partial sum, p and ds of the fused backward is exact in fp32 and in either 16-bit format,
    so that the ONLY rounding left is the output's.  All fp64, integer valued:
        q_i = a_i e_0 + a'_i e_300, k_j = b_j e_0 + b'_j e_300      s_ij = a_i b_j + a'_i b'_j, an integer
        L_i = max_j possible s_ij + off_i                           p_ij = 2^(s_ij - L_i), a power of two in [2^-6, 1]
        do_i: two non-zeros in {+-1, +-2, +-3} at channels c_i = (7 i + 3) mod 512 and c_i + 256: one in each half, and for N <= 256 no two
              rows share a channel;  v, o: integers in [-3, 3] and [-2, 2] that depend on (row, channel) -- dp_ij and D_i are two-term sums
    Rows are distinguishable: a, a', off, the positions and values of do, and v / o change with the row (rows i and i + 8, which a lane
    shuffle could confuse, differ in L); every image differs (the row index runs on across the batch).  N <= 256 uses the whole range
    of p; above it several rows share a channel of dv, and the range is [2^-2, 1] with |do| <= 2 so that one term stays visible next
    to the others in 8 significant bits (single_term_sensitivity asserts it)."""
    wide = N <= 256
    r = (torch.arange(B * N).view(B, N) + 5 * torch.arange(B).view(B, 1)).double()          # the row index, running on across the batch
    c = torch.arange(512).double()
    if wide:
        a, a2, off = 1 + r % 2, 1 - 2 * ((r // 2) % 2), (r // 8) % 2
        b, b2 = r % 3, (r // 3) % 2
        Lmax = 2 * a + a2.clamp_min(0)                                                      # b <= 2, b' <= 1
    else:
        a, a2, off = 1 - 2 * (r % 2), 1 - 2 * ((r // 8) % 2), torch.zeros_like(r)
        b, b2 = r % 2, (r // 2) % 2
        Lmax = a.clamp_min(0) + a2.clamp_min(0)
    q, k = torch.zeros(B, N, 512, dtype=torch.float64), torch.zeros(B, N, 512, dtype=torch.float64)
    q[..., EXACT_CH[0]], q[..., EXACT_CH[1]] = a, a2
    k[..., EXACT_CH[0]], k[..., EXACT_CH[1]] = b, b2
    L = Lmax + off
    do = torch.zeros(B, N, 512, dtype=torch.float64)
    ch = ((7 * r + 3) % 512).long()
    top = 3 if wide else 2
    val1 = (1 + r % top) * (1 - 2 * ((r // 3) % 2))
    val2 = (1 + (r // 2) % top) * (1 - 2 * ((r // 5) % 2))
    do.scatter_(2, ch.unsqueeze(-1), val1.unsqueeze(-1))
    do.scatter_(2, ((ch + 256) % 512).unsqueeze(-1), val2.unsqueeze(-1))
    rr = r.unsqueeze(-1)
    v = (rr * (2 * c + 1) + c) % 7 - 3
    o = (rr + 3 * c) % 5 - 2
    return q, k, v, o, do, L


def _ulp(v, m, emin):
    """the spacing of the 16-bit format (m mantissa bits, smallest normal exponent emin) at |v|"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin)))
    e = torch.where(torch.exp2(e) > v.abs().clamp_min(2.0 ** emin), e - 1, e)
    return torch.exp2(e.clamp_min(emin) - m)


def exact_attention_bounds(q, k, v, o, do, L, m, emin, n_u=3.0):
    """-> (dq, dk, dv exact), (their bounds 0.5 ulp16(exact) + n_u U sum |terms|), (p, ds)"""
    U = 2.0 ** -24
    _, p, _, _, ds = attention_backward_terms(q, k, v, o, do, L, 1.0)
    exact = (ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do)
    mags = (ds.abs() @ k.abs(), ds.abs().transpose(-1, -2) @ q.abs(), p.transpose(-1, -2) @ do.abs())
    return exact, tuple(0.5 * _ulp(e, m, emin) + n_u * U * g for e, g in zip(exact, mags)), (p, ds)


def single_term_sensitivity(q, k, do, p, ds, bounds):
    """[B, N, N]: for every (i, j), the largest |change| / bound over the output elements that the term (i, j) feeds when it alone is
    removed from the sums: dv_j[c] loses p_ij do_i[c], dk_j[c] loses ds_ij q_i[c], dq_i[c] loses ds_ij k_j[c]"""
    bq, bk, bv = bounds
    best = torch.zeros_like(p)
    for c in EXACT_CH:                                                        # q and k are zero elsewhere
        best = torch.maximum(best, ds.abs() * q[..., c].abs().unsqueeze(-1) / bk[..., c].unsqueeze(-2))
        best = torch.maximum(best, ds.abs() * k[..., c].abs().unsqueeze(-2) / bq[..., c].unsqueeze(-1))
    assert int((do != 0).sum(-1).max()) <= 2
    val, idx = do.abs().topk(2, dim=-1)                                       # the two non-zeros of row i: dv_j[idx] is what it feeds
    img = torch.arange(do.shape[0], device=do.device).view(-1, 1)
    for t in range(2):
        best = torch.maximum(best, p * val[..., t:t + 1] / bv.transpose(1, 2)[img, idx[..., t]])
    return best
