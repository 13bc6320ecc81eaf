"""CPU: tests/flow_fused_fp64.py, the reference of test_gpu_flow_fused_edges.py.
  1. the restatement against oracle.torch_ref.FlowStep(3, coupling=True) in double, reverse=True, with non-zero Conv2dZeros weights and logs and
     non-trivial ActNorms, the operands derived as FlowUpsamplerNet._prepare derives them (folded(), reverse_affine_fp64(), ftA and hF from the
     oracle's own fAffine[0] / fFeatures on ft), at every image size the GPU file launches: to fp64 noise;
  2. the exact family is representable in both 16-bit formats -- every hi / lo pair exact, every dropped sum zero, every sum of magnitudes below
     2^24 of its unit (flow_fused_fp64.exact_report) -- and not degenerate: every tap, every one of the 64 + 64 channels and every one of the 36
     S rows carries a non-zero filter entry, at least a third of h2 is positive, sigmoid(h4 + 2) + eps >= 0.25; the "act_lo", "wz_lo", "w2_lo"
     and "w4_lo" variants do carry non-zero lo halves (activations; each of the three filters in turn);
  3. sensitivity: every mutation of flow_fused_fp64.MUTATIONS moves the exact family's expected z_out by more than the exact family's bound at
     some element, and exceeds the random family's bound at some element -- so no GPU run is needed to see the GPU test fail.
     The two dropped-product mutations need a lo to drop: on the exact family they are shown on "act_lo" (w_hi . x_lo) and on "wz_lo" / "w2_lo" /
     "w4_lo" (w_lo . x_hi in the first / second / third product), in BOTH formats, by hundreds of times the bound.  On the random family they
     exceed the bound under bf16 (a lo is 2^-9 of its hi: the missing product is ~2^-9 of a contraction, the bound ~2^-11 of it) and do NOT under fp16 (a lo is 2^-12 of its hi, below the worst-case fp32 accumulation
     count 2 U (3 K + 1) = 2^-15.4 x 64 terms' magnitudes): under fp16 only the exact family tells the fp32-class form from a plain 16-bit one.
     That is asserted, so the statement stays true.  `eps_omitted` on the random family is shown at the second eps the GPU file runs (0.3): at
     1e-4 eps moves z by 1e-4 relative, below the random family's worst-case bound (~1e-3 relative, the propagation through |W2| |W4|), while
     the exact family sees it there by hundreds of times its bound."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_fused_fp64 as R
from oracle import torch_ref as O

FU = importlib.import_module("glare_amd.modules.FlowUpsamplerNet")   # the module (the package re-exports the class under this name)
SENS = (2, 17, 41)          # 2 x 2 tiles, two images: every mechanism a mutation touches exists
FAR_EPS = 0.3
IDS = {torch.bfloat16: "bf16", torch.float16: "fp16"}


def _oracle_step(seed):
    """an oracle FlowStep in double with every parameter away from its trivial value, and the same weights in the project's containers"""
    torch.manual_seed(seed)
    np.random.seed(seed)
    st = O.FlowStep(3, coupling=True).double().eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in st.named_parameters():
            if name.endswith("logs"):
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.1)
            elif name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.3)
            elif name == "invconv.weight":
                p.add_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.1)
            else:          # conv weights, the Conv2dZeros ones included
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.05)
    mine = FU.FlowStep(3).double().eval()
    mine.load_state_dict(st.state_dict())
    return st, mine


@pytest.mark.parametrize("size", R.SIZES, ids=["%dx%dx%d" % s for s in R.SIZES])
def test_restatement_against_the_oracle_flow_step(size):
    B, H, W = size
    st, mine = _oracle_step(B + H + W)
    g = torch.Generator().manual_seed(H * 100 + W)
    z = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64) * 0.7
    ft = torch.sigmoid(torch.randn(B, 64, H, W, generator=g, dtype=torch.float64))
    with torch.no_grad():
        # FlowStep.forward(reverse=True) in its own order; the oracle's invconv rounds its inverse to fp32 (Permutations.py:38), which a double
        # input does not take, so that one layer is applied here with the fp64 inverse
        want, _ = st.affine(z, torch.zeros(B, dtype=torch.float64), True, ft)
        want = F.conv2d(want, torch.inverse(st.invconv.weight).view(3, 3, 1, 1))
        want, _ = st.actnorm(want, None, True)
        aff = mine.affine
        w0, b0 = aff.fAffine[0].folded()
        ftA = F.conv2d(ft, w0[:, 1:], b0, 1, 1).permute(0, 2, 3, 1)
        hF = F.pad(st.affine.fFeatures(ft).permute(0, 2, 3, 1), (0, 2))
        (w2, b2), (w4, b4) = aff.fAffine[2].folded(), aff.fAffine[4].folded()
        A, c = mine.reverse_affine_fp64()
    o = dict(z=z.permute(0, 2, 3, 1).contiguous(), ftA=ftA, wz=w0[:, 0].reshape(64, 9), w2=w2.reshape(64, 64), b2=b2, w4=w4, b4=b4, hF=hF, M=A, t=c,
             eps=float(aff.affine_eps), family="random")
    for dtype in R.FORMATS:          # the value does not depend on the format; the bound does
        got, bound, hid = R.step_fp64(o, dtype)
        assert float(hid["h4"].abs().max()) > 0.05          # the Conv2dZeros is not a zero
        err = float((got - want.permute(0, 2, 3, 1)).abs().max())
        assert err < 1e-12 * max(1.0, float(want.abs().max())), err
        assert bool((bound > 0).all()) and bool(torch.isfinite(bound).all())


@pytest.mark.parametrize("dtype", R.FORMATS, ids=IDS.values())
@pytest.mark.parametrize("variant", R.EXACT_VARIANTS)
def test_exact_family_is_representable_and_not_degenerate(variant, dtype):
    for B, H, W in R.SIZES:
        o = R.exact_operands(B, H, W, variant, dtype)
        rep, hid = R.exact_report(o, dtype)
        assert rep["pairs"] == 0.0 and rep["dropped"] == 0.0 and rep["replay"] == 0.0 and rep["whole"], (variant, dtype, (B, H, W), rep)
        assert max(rep["mags"]) < 2.0 ** 24, rep["mags"]
        assert (rep["lo_w"] > 0) == (variant in ("wz_lo", "w2_lo", "w4_lo")) and (rep["lo_x"] > 0) == (variant in ("act_lo", "wz_lo", "w2_lo")), (rep["lo_w"], rep["lo_x"])
        for n in ("z", "ftA", "wz", "w2", "b2", "w4", "b4", "hF", "M", "t"):
            assert o[n].dtype == torch.float32          # what the ABI receives
        wz, w2, b2, w4r, b4 = R.filters(o)
        assert bool((wz != 0).any(0).all()) and bool((wz != 0).any(1).all())           # 9 taps, 64 h1 channels
        assert bool((w2 != 0).any(0).all()) and bool((w2 != 0).any(1).all())           # 64 h1 channels in, 64 h2 channels out
        assert bool((w4r != 0).any(0).all()) and bool((w4r != 0).any(1).all())         # 64 h2 channels, 36 S rows
        assert bool((o["z"][..., 0] != 0).all())
        h2 = hid["h2"][:, 1:H + 1, 1:W + 1]
        assert float((h2 > 0).double().mean()) >= 1.0 / 3.0, (variant, (B, H, W))
        assert float(hid["h2"].abs().max()) < 128.0          # 7 integer bits: with 9 fraction bits still a bf16 pair
        assert float((torch.sigmoid(hid["h4"][..., 1::2] + 2.0) + o["eps"]).min()) >= 0.25
        if B > 1:          # every image has its own pattern
            assert not torch.equal(o["z"][0, ..., 0], o["z"][1, ..., 0]) or H * W == 1
            assert not torch.equal(o["ftA"][0], o["ftA"][1])


def test_exact_bound_is_the_tail_alone():
    """with h4 exact the bound of a step is a few fp32 roundings of the tail: nothing of the 16-bit format is in it"""
    o = R.exact_operands(*SENS, "act_lo", torch.bfloat16)
    out, b_bf, _ = R.step_fp64(o, torch.bfloat16)
    _, b_fp, _ = R.step_fp64(o, torch.float16)
    assert torch.equal(b_bf, b_fp)
    _, loose, _ = R.step_fp64(o, torch.bfloat16, h4_exact=False)
    assert bool((loose > b_bf).all())
    M, t = o["M"].double().abs(), o["t"].double().abs()
    assert bool((b_bf <= 40 * R.U * (_tail_magnitudes(o, out) @ M.t() + t)).all())


def _tail_magnitudes(o, out):
    """|z0|, |z1|, |z2| before M, with the magnitudes of what was subtracted on the way: the scale of the tail's roundings"""
    hid = R.hidden(o, torch.bfloat16)
    z, f, h4, eps = o["z"].double(), o["hF"].double(), hid["h4"], o["eps"]
    s = lambda a: torch.sigmoid(a + 2.0) + eps
    q1 = (z[..., 1].abs() / s(h4[..., 1]) + h4[..., 0].abs()) / s(f[..., 3]) + f[..., 2].abs()
    q2 = (z[..., 2].abs() / s(h4[..., 3]) + h4[..., 2].abs()) / s(f[..., 5]) + f[..., 4].abs()
    return torch.stack([z[..., 0].abs() / s(f[..., 1]) + f[..., 0].abs(), q1, q2], -1)


def _exceeds(o, dtype, mutation):
    out, bound, _ = R.step_fp64(o, dtype)
    mut, _, _ = R.step_fp64(o, dtype, mutation)
    return float(((mut - out).abs() / bound).max())


@pytest.mark.parametrize("dtype", R.FORMATS, ids=IDS.values())
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_moves_the_exact_family(mutation, dtype):
    variants = {"wlo_xhi_dropped": ("wz_lo", "w2_lo", "w4_lo"), "whi_xlo_dropped": ("act_lo", "wz_lo", "w2_lo")}.get(mutation, R.EXACT_VARIANTS)
    for variant in variants:
        r = _exceeds(R.exact_operands(*SENS, variant, dtype), dtype, mutation)
        assert r > 100.0, (mutation, variant, r)          # a unit of h4, or a whole operand, against a few fp32 roundings
    if mutation in R.DROPPED:          # nothing to drop where every lo is zero
        assert _exceeds(R.exact_operands(*SENS, "int", dtype), dtype, mutation) == 0.0


@pytest.mark.parametrize("dtype", R.FORMATS, ids=IDS.values())
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_exceeds_the_random_bound(mutation, dtype):
    eps = FAR_EPS if mutation == "eps_omitted" else R.FLOW_EPS
    r = _exceeds(R.random_operands(*SENS, eps=eps), dtype, mutation)
    if mutation in R.DROPPED and dtype == torch.float16:
        assert 0.05 < r < 1.0, (mutation, r)          # the module docstring says why; the exact family's "act_lo" / "wz_lo" see these under fp16
    else:
        assert r > 1.5, (mutation, r)


def test_mutations_that_need_a_seam_or_a_border_are_silent_without_one():
    """the restatement's own geometry: in one tile, one image, nothing reads another tile's pixel; on a 1 x 1 image every halo pixel is outside"""
    o = R.exact_operands(1, 16, 40, "int")
    out, _, _ = R.step_fp64(o, torch.bfloat16)
    assert torch.equal(R.step_fp64(o, torch.bfloat16, "halo_from_previous_image")[0], out)
    o = R.exact_operands(3, 1, 1, "int")
    out, bound, _ = R.step_fp64(o, torch.bfloat16)
    for m in ("h2_not_zeroed", "z0_clamped"):
        assert float(((R.step_fp64(o, torch.bfloat16, m)[0] - out).abs() / bound).max()) > 100.0, m
