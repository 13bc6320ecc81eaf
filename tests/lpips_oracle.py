"""LPIPS on VGG16 (Zhang et al. 2018; the `lpips` package 0.1.x, taming's `LPIPS`) restated in plain torch from the published definition --
the module is not in the reference tree: scaling layer, five VGG16 slices (torchvision cfg 'D', taps after relu1_2 .. relu5_3),
normalize_tensor, the 1x1 heads, the spatial average, the sum over the taps.  NCHW, fp32 (or whatever dtype it is moved to), CPU.
State-dict keys and shapes are the published files'.

`emulate=torch.float16 | torch.bfloat16`: the same network with a tensor rounded to that format wherever the HIP training path stores
16 bits -- every conv + ReLU output (a pooled map of rounded values is exact), every activation gradient (the head's included: formed in
fp32, rounded once), and the filters (plain round-to-nearest; the first conv reads its fp32 filter).  EMULATED_ERR holds what that
rounding alone does to the value and to d / dxrec: the source of the network-level bounds of tests/test_gpu_lpips.py, checked on the CPU
by tests/test_lpips_host.py.  A plain module like disc_oracle.py."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
CHANNELS = (64, 128, 256, 512, 512)
EPS = 1e-10
NET_SHAPES = ((2, 64, 64), (1, 32, 48), (1, 16, 16))     # relu5_3: 4 x 4, 2 x 3, 1 x 1
NET_SEEDS = (11, 12, 13)
EMU_LOSS_SCALE = {torch.float16: 4096.0, torch.bfloat16: 1.0}     # tests/test_gpu_stage1.py LOSS_SCALE: what scale_loss does for fp16 gradients

# Largest relative L2 error over NET_SEEDS x NET_SHAPES of the emulated network against the fp32 one (value: |v - v32| / |v32| of the
# batch mean), as emulation_errors() computes it, rounded up in the third digit.  tests/test_lpips_host.py recomputes it on the CPU and
# holds this table to the computation (not below it, at most 2 % above); tests/test_gpu_lpips.py doubles it.
# fp16's gradient error is not bf16's / 8: behind 13 ReLUs and 4 max-pools on seeded filters it is mostly decisions flipped by the
# rounding, not the rounding itself.
EMULATED_ERR = {"fp16": {"value": 1.98e-4, "dx": 5.41e-2},
                "bf16": {"value": 2.56e-3, "dx": 0.156}}


class _Round16(torch.autograd.Function):
    """forward: the value rounded to the 16-bit format; backward: the gradient rounded to it."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


def _r16(x, dtype):
    return x if dtype is None else _Round16.apply(x, dtype)


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.tensor([.458, .448, .450])[None, :, None, None])

    def forward(self, inp):
        return (inp - self.shift) / self.scale


class NetLinLayer(nn.Module):
    def __init__(self, chn):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn, 1, 1, stride=1, padding=0, bias=False))


def normalize_tensor(x, eps=EPS):
    norm = torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True))
    return x / (norm + eps)


def head(a, b, w, eps=EPS):
    """One tap: feature maps a, b [B, C, H, W], head weights w [C] -> [B]: spatial_average(lin((normalize(a) - normalize(b))^2))."""
    d = (normalize_tensor(a, eps) - normalize_tensor(b, eps)) ** 2
    return (d * w.view(1, -1, 1, 1)).sum(dim=1, keepdim=True).mean(dim=(2, 3)).reshape(-1)


class LPIPS(nn.Module):
    def __init__(self):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.net = nn.Module()
        cin, nxt = 3, 0
        for k, (idx, cout) in enumerate(zip(SLICES, CHANNELS)):
            sl = nn.Sequential()
            if k:
                sl.add_module(str(nxt), nn.MaxPool2d(kernel_size=2, stride=2))
            for i in idx:
                sl.add_module(str(i), nn.Conv2d(cin, cout, 3, padding=1))
                sl.add_module(str(i + 1), nn.ReLU(inplace=False))
                cin = cout
            nxt = idx[-1] + 2
            setattr(self.net, "slice%d" % (k + 1), sl)
            setattr(self, "lin%d" % k, NetLinLayer(cout))
        self.eval()
        for p in self.parameters():
            p.requires_grad = False

    def features(self, img01, emulate=None):
        """img01: NCHW in [0, 1] -> the five taps."""
        h, feats = self.scaling_layer(2 * img01 - 1), []
        for k in range(5):
            for m in getattr(self.net, "slice%d" % (k + 1)):
                if isinstance(m, nn.Conv2d):
                    w = m.weight if (emulate is None or m.in_channels == 3) else m.weight.to(emulate).to(m.weight.dtype)
                    h = F.conv2d(h, w, m.bias, padding=1)
                elif isinstance(m, nn.ReLU):
                    h = _r16(torch.relu(h), emulate)
                else:
                    h = m(h)
            h = _r16(h, emulate)      # the tap feeds the head and the next slice: their two gradients meet in one 16-bit sum
            feats.append(h)
        return feats

    def per_image(self, xrec, x, emulate=None):
        fa = self.features(xrec, emulate)
        with torch.no_grad():
            fb = self.features(x, emulate)
        total = 0
        for k, (a, b) in enumerate(zip(fa, fb)):
            w = getattr(self, "lin%d" % k).model[1].weight.reshape(-1)
            total = total + head(_r16(a, emulate), b, w)
        return total

    def forward(self, xrec, x, emulate=None):
        """The batch mean of the per-image distance: `mean(p_loss)` of taming's nll_loss."""
        return self.per_image(xrec, x, emulate).mean()


def seeded_state(seed):
    """Name-seeded weights (glare_amd.synthetic.seeded_init_) in a regime where all five taps carry signal: the conv filters scaled by
    sqrt(6) (uniform +-sqrt(6 / fan_in): activations keep their scale through conv + ReLU; the default +-1 / sqrt(fan_in) shrinks them
    by 0.4 per layer, and relu5_3 would hold the biases alone), the heads non-negative as the published ones are."""
    from glare_amd.synthetic import seeded_init_

    const = LPIPS().state_dict()
    sd = {k: v.clone() for k, v in seeded_init_(LPIPS(), seed).state_dict().items()}
    for k in sd:
        if k.startswith("scaling_layer."):
            sd[k] = const[k].clone()                              # the definition's constants, not weights
        elif k.startswith("net.") and k.endswith(".weight"):
            sd[k] = sd[k] * math.sqrt(6.0)
        elif k.startswith("lin"):
            sd[k] = sd[k].abs() * math.sqrt(sd[k].shape[1])      # U(0, 1): the published heads are of that order
    return sd


def torchvision_form(sd):
    """(backbone under torchvision's `features.N.*` keys, heads under `linK.model.1.weight`) of an LPIPS state dict."""
    back = {"features." + k.split(".", 2)[2]: v for k, v in sd.items() if k.startswith("net.")}
    return back, {k: v for k, v in sd.items() if k.startswith("lin")}


def net_case(seed, shape):
    """(xrec, x) NCHW in [0, 1]: a reconstruction-like pair, x and x + noise of 10 %."""
    g = torch.Generator().manual_seed(1000 + seed)
    B, H, W = shape
    x = torch.rand(B, 3, H, W, generator=g)
    xrec = (x + 0.1 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1)
    return xrec, x


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def emulation_errors(dtype):
    """{quantity: largest rel-L2 error over NET_SEEDS x NET_SHAPES} of the rounding emulation against the fp32 oracle."""
    worst = {"value": 0.0, "dx": 0.0}
    s = EMU_LOSS_SCALE[dtype]
    for seed in NET_SEEDS:
        net = LPIPS()
        net.load_state_dict(seeded_state(seed))
        for shape in NET_SHAPES:
            xrec, x = net_case(seed, shape)
            out = {}
            for emu in (None, dtype):
                xr = xrec.clone().requires_grad_(True)
                v = net(xr, x, emulate=emu)
                (g,) = torch.autograd.grad(v * (s if emu is not None else 1.0), xr)
                g = g / (s if emu is not None else 1.0)
                out[emu] = (v.detach(), g)
            worst["value"] = max(worst["value"], rel(out[dtype][0], out[None][0]))
            worst["dx"] = max(worst["dx"], rel(out[dtype][1], out[None][1]))
    return worst


# What the LPIPS term's 16-bit rounding ALONE does to the parameter gradients of a stage-1 step (fp32 autoencoder, loss = l1 + lpips +
# codebook term, 1 x 3 x 64 x 64, seed 11): the rel-L2 error per parameter tensor of the step with the emulated LPIPS against the step
# with the fp32 one, (median, largest), as step_emulation_errors() computes it, rounded up in the third digit and held to the
# computation by tests/test_lpips_host.py as EMULATED_ERR is.  The error of the seed d (l1 + lpips) / dxrec is carried through the
# oracle's own backward, so what the 3-channel bottleneck does to it is in the figure: the largest is quant_conv / post_quant_conv's.
EMULATED_STEP_ERR = {"fp16": (0.0265, 0.116), "bf16": (0.0799, 0.576)}


def step_case(seed):
    """(oracle VQModel, x, LPIPS oracle) of the trainer-step tests: the autoencoder name-seeded with 6, the codebook redrawn N(0, sigma)."""
    from glare_amd.synthetic import seeded_init_
    from oracle import torch_ref as O

    g = torch.Generator().manual_seed(seed)
    ref = seeded_init_(O.VQModel().train(), 6)
    x = torch.rand(1, 3, 64, 64, generator=g)
    with torch.no_grad():
        sigma = float(ref.encode(x)[0].std())
    E = torch.randn(8192, 3, generator=g) * sigma
    ref.quantize.embedding.weight.data.copy_(E)
    lp = LPIPS()
    lp.load_state_dict(seeded_state(seed))
    return ref, x, E, lp


STEP_LOSS_SCALE = {torch.float16: 1024.0, torch.bfloat16: 1.0}     # the GradScaler's scale the trainer-step tests set


def term_rounding_errors(dtype, named, rest, dec, x, lp):
    """{parameter name: rel-L2 error of d (rest + lp(dec, x)) / d parameter with the emulated LPIPS against the same with the fp32 one}:
    what the term's 16-bit rounding alone does to each gradient of a step whose other terms are `rest` and whose reconstruction is `dec`."""
    s = STEP_LOSS_SCALE[dtype]
    grads = {}
    for emu in (None, dtype):
        k = s if emu is not None else 1.0
        loss = (rest + lp(dec, x, emulate=emu)) * k
        grads[emu] = [None if g is None else g / k for g in torch.autograd.grad(loss, [p for _, p in named], allow_unused=True, retain_graph=True)]
    return {n: rel(a, b) for (n, _), a, b in zip(named, grads[dtype], grads[None]) if b is not None and not n.endswith(".k.bias")}


def step_emulation_errors(dtype, seed=11):
    ref, x, _, lp = step_case(seed)
    dec, rq, _ = ref.decode(ref.encode(x)[0])
    gen = [(n, p) for n, p in ref.named_parameters() if not n.startswith("conv_semantic.")]
    errs = sorted(term_rounding_errors(dtype, gen, (dec - x).abs().mean() + rq, dec, x, lp).values())
    return errs[len(errs) // 2], errs[-1]
