"""CPU oracles of the patch discriminator (tests only; a plain module like tolerances.py).

  sequential()      taming's NLayerDiscriminator.main restated as a plain torch.nn.Sequential (the specification of glare_amd.modules.
                    discriminator): the state-dict keys, the fp32 autograd reference of the whole network.
  conv4x4_64()      the 4x4 / pad 1 conv, its two gradients and the magnitude sums of their terms in fp64 (torch's own conv + autograd).
  bn_forward_64()   BatchNorm2d (training mode, per batch group) + LeakyReLU(0.2) in fp64 with the fp32 evaluation error of
  bn_backward_64()  csrc/disc_ops.hip's expressions, counted per step (U = one fp32 rounding).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

U = 2.0 ** -24
SLOPE = float(torch.tensor(0.2, dtype=torch.float32))       # the kernels' 0.2f


def sequential(input_nc=3, ndf=64, n_layers=3):
    seq = [nn.Conv2d(input_nc, ndf, 4, 2, 1), nn.LeakyReLU(0.2)]
    mult = 1
    for n in range(1, n_layers):
        prev, mult = mult, min(2 ** n, 8)
        seq += [nn.Conv2d(ndf * prev, ndf * mult, 4, 2, 1, bias=False), nn.BatchNorm2d(ndf * mult), nn.LeakyReLU(0.2)]
    prev, mult = mult, min(2 ** n_layers, 8)
    seq += [nn.Conv2d(ndf * prev, ndf * mult, 4, 1, 1, bias=False), nn.BatchNorm2d(ndf * mult), nn.LeakyReLU(0.2)]
    seq += [nn.Conv2d(ndf * mult, 1, 4, 1, 1)]
    return nn.Sequential(*seq)


class Discriminator(nn.Module):
    """The Sequential under taming's attribute name: state-dict keys main.0.weight, main.3.running_mean, ..."""

    def __init__(self, input_nc=3, ndf=64, n_layers=3):
        super().__init__()
        self.main = sequential(input_nc, ndf, n_layers)

    def forward(self, x):
        return self.main(x)


def lrelu64(z):
    return torch.where(z > 0, z, SLOPE * z)


def conv4x4_64(x_nhwc, w_oihw, bias, g_nhwc, stride):
    """fp64 on the CPU.  -> dict: y (pre-activation incl. bias), ymag = sum |x w| + |b|, dx, dxmag = sum |g w|, dw, dwmag = sum |g x|,
    db, dbmag = sum |g|; all NHWC / OIHW."""
    x = x_nhwc.double().cpu().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w = w_oihw.double().cpu().clone().requires_grad_(True)
    b = None if bias is None else bias.double().cpu()
    out = {}
    y = F.conv2d(x, w, None, stride, 1)
    out["y"] = (y if b is None else y + b.view(1, -1, 1, 1)).detach().permute(0, 2, 3, 1).contiguous()
    ymag = F.conv2d(x.detach().abs(), w.detach().abs(), None, stride, 1)
    out["ymag"] = (ymag if b is None else ymag + b.abs().view(1, -1, 1, 1)).permute(0, 2, 3, 1).contiguous()
    if g_nhwc is not None:
        g = g_nhwc.double().cpu().permute(0, 3, 1, 2).contiguous()
        dx, dw = torch.autograd.grad(y, (x, w), g)
        xa, wa = x.detach().abs().requires_grad_(True), w.detach().abs().requires_grad_(True)
        dxm, dwm = torch.autograd.grad(F.conv2d(xa, wa, None, stride, 1), (xa, wa), g.abs())
        out.update(dx=dx.permute(0, 2, 3, 1).contiguous(), dxmag=dxm.permute(0, 2, 3, 1).contiguous(), dw=dw, dwmag=dwm,
                   db=g.sum((0, 2, 3)), dbmag=g.abs().sum((0, 2, 3)))
    return out


def _grouped(t, groups):
    """[B, H, W, C] -> [G, n, C]"""
    return t.reshape(groups, -1, t.shape[-1])


def bn_forward_64(x, gamma, beta, groups, eps, lrelu=True):
    """x [B, H, W, C] (16-bit values), gamma / beta fp32 -> fp64 (y, mean [G, C], var, rstd) and the error bounds (e_y like y, e_mean, e_var,
    e_rstd) of the kernels' evaluation:
      mean  a sum of n terms in some fixed order, then one division:       e_mean = U (sum |x| (n - 1) / n + |mean|)
      d = x - mean', d^2, their sum, / n (two-pass):                        e_var  = mean(2 |d| e_mean + 3 U d^2) + e_mean^2 + n U var + U var
      rstd = 1 / sqrt(var + eps):                                           e_rstd = rstd (0.5 (e_var + U (var + eps)) / (var + eps) + 2 U)
      xhat = (x - mean) rstd:                                               e_xhat = (e_mean + U |d|) rstd + |d| e_rstd + U |xhat|
      z = fma(xhat, gamma, beta); y = lrelu(z) (1-Lipschitz, one product):  e_y    = |gamma| e_xhat + U (|gamma xhat| + |beta|) + U |z|"""
    x = _grouped(x.double().cpu(), groups)
    ga, be = gamma.double().cpu(), beta.double().cpu()
    n = x.shape[1]
    mean = x.mean(1)
    d = x - mean[:, None]
    var = (d * d).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    e_mean = U * (x.abs().sum(1) * (n - 1) / n + mean.abs())
    e_var = (2 * d.abs() * e_mean[:, None] + 3 * U * d * d).mean(1) + e_mean ** 2 + (n + 1) * U * var
    e_rstd = rstd * (0.5 * (e_var + U * (var + eps)) / (var + eps) + 2 * U)
    xhat = d * rstd[:, None]
    e_xhat = (e_mean[:, None] + U * d.abs()) * rstd[:, None] + d.abs() * e_rstd[:, None] + U * xhat.abs()
    z = xhat * ga + be
    y = lrelu64(z) if lrelu else z
    e_y = ga.abs() * e_xhat + U * ((ga * xhat).abs() + be.abs()) + U * z.abs()
    return (y, mean, var, rstd), (e_y, e_mean, e_var, e_rstd)


def bn_backward_64(x, dy, saved, gamma, beta, groups, lrelu=True):
    """The backward on the kernel's OWN saved statistics (fp32 values, exact inputs here).  -> fp64 (dx [G, n, C], dgamma [C], dbeta [C]) and
    their bounds.  Per element, xhat = (x - mean) rstd rounds twice (e_xhat = 2 U |xhat|); the activation's derivative is decided by the sign
    of z = fma(xhat, gamma, beta), whose fp32 value can differ from the exact one by e_z = |gamma| e_xhat + U (|gamma xhat| + |beta|): where
    |z| <= e_z either side of the kink is a correct answer and the bound takes the 0.8 |dy| between them (`amb`).
      dz = dy or 0.2 dy (one product):                      e_dz = U |dz| + amb 0.8 |dy|
      sb = sum dz, sg = sum dz xhat (fma chain), n terms:   e_sb = n U sum |dz| + sum e_dz;   e_sg = n U sum |dz xhat| + sum (|dz| e_xhat + e_dz |xhat|)
      dbeta / dgamma = the groups' sums in group order:     + G U on the magnitudes
      mb = sb / n, mg = sg / n (one division each), t = (dz - mb) - xhat mg (three roundings), c = gamma rstd (one), dx = c t (one)"""
    x, dy = _grouped(x.double().cpu(), groups), _grouped(dy.double().cpu(), groups)
    saved = saved.double().cpu()
    mean, rstd = saved[:, 0], saved[:, 1]
    ga, be = gamma.double().cpu(), beta.double().cpu()
    n, G = x.shape[1], groups
    xhat = (x - mean[:, None]) * rstd[:, None]
    e_xhat = 2 * U * xhat.abs()
    z = xhat * ga + be
    e_z = ga.abs() * e_xhat + U * ((ga * xhat).abs() + be.abs())
    if lrelu:
        dz = torch.where(z > 0, dy, SLOPE * dy)
        amb = (z.abs() <= e_z).double()
    else:
        dz, amb = dy, torch.zeros_like(dy)
    e_dz = U * dz.abs() + amb * 0.8 * dy.abs()
    sb, sg = dz.sum(1), (dz * xhat).sum(1)
    sb_mag, sg_mag = dz.abs().sum(1), (dz * xhat).abs().sum(1)
    e_sb = n * U * sb_mag + e_dz.sum(1)
    e_sg = n * U * sg_mag + (dz.abs() * e_xhat + e_dz * xhat.abs()).sum(1)
    dbeta, dgamma = sb.sum(0), sg.sum(0)
    e_dbeta, e_dgamma = e_sb.sum(0) + G * U * sb_mag.sum(0), e_sg.sum(0) + G * U * sg_mag.sum(0)
    mb, mg = sb / n, sg / n
    e_mb, e_mg = e_sb / n + U * mb.abs(), e_sg / n + U * mg.abs()
    t = dz - mb[:, None] - xhat * mg[:, None]
    t_mag = dz.abs() + mb.abs()[:, None] + (xhat * mg[:, None]).abs()
    e_t = e_dz + e_mb[:, None] + mg.abs()[:, None] * e_xhat + xhat.abs() * e_mg[:, None] + 3 * U * t_mag
    c = ga * rstd
    dx = c[:, None] * t
    e_dx = c.abs()[:, None] * e_t + 2 * U * c.abs()[:, None] * t_mag
    return (dx, dgamma, dbeta), (e_dx, e_dgamma, e_dbeta)
