"""CPU: tests/dcn_fp64.py, the reference of test_gpu_dcn_edges.py.
  1. the restatement against the C oracle (oracle.c_ref.dcn_forward, fp32) on every geometry the GPU file launches -- to fp32 noise on the
     random family, bit for bit on the exact family -- against F.conv2d at zero offset / unit mask, and against F.conv2d of an
     integer-shifted, zero-filled input at integer offsets;
  2. the exact family is representable: every sample a multiple of 1/64 (1/8 narrow) that bf16 holds, every sum of magnitudes of an output
     below 2^24 / 64 and of a whole tile too, and it is not a field of zeros: every tap, deformable group, 8-channel chunk and output
     channel carries a non-zero filter tap;
  3. the comparisons are sensitive: every mutation of dcn_fp64.MUTATIONS changes the exact family's expected values and exceeds the bound on the
     random family -- but the two that turn the in-image rule's > / < into >= / <= at h = -1 / h = H, which change NOTHING: with per-corner
     dropping the rule decides nothing of its own at its limits (dcn_fp64.SILENT has the argument).  That is asserted as well."""
import numpy as np
import pytest
import torch

import dcn_fp64 as D
from oracle import c_ref

def _geoms():
    """every geometry test_gpu_dcn_edges.py launches: the lean instantiations, the general kernel's, the drop-in's MFMA and generic ones"""
    out = [dict(name=c["name"], C=c["C"], Co=c["Co"], dg=c["dg"], narrow=c["single"]) for c in D.LEAN]
    out += [dict(name="general-C%d-Co%d-dg%d" % (c["C"], c["Co"], c["dg"]), C=c["C"], Co=c["Co"], dg=c["dg"]) for c in D.GENERAL]
    out += [dict(c, name="drop-in-" + c["name"]) for c in D.DROP_IN]
    return out


GEOMS = _geoms()


def _oracle(o, bias=True):
    k, s, p, d, dg, groups = o["geom"]
    B = o["x"].shape[0]
    Ho, Wo = D.out_size(o["x"].shape[1], o["x"].shape[2], k, s, p, d)
    m = D.mask_values(o["mask"], o["is_logit"]).float()
    y = c_ref.dcn_forward(o["x"].permute(0, 3, 1, 2).numpy(), o["offset"].view(B, -1, Ho, Wo).numpy(), m.view(B, -1, Ho, Wo).numpy(), o["w"].numpy(),
                          o["bias"].numpy() if bias else None, stride=s, padding=p, dilation=d, groups=groups, dg=dg)
    return torch.from_numpy(np.ascontiguousarray(y)).permute(0, 2, 3, 1).double()


def _sizes(g):
    """the image sizes the GPU file runs a geometry on: dcn_fp64.SIZES, the planar test's 5 x 5 at B = 4, a GENERIC_CASES entry's own size"""
    return list(zip(D.SIZES, (1, 3, 1, 3, 1, 3))) + [(D.PLANAR[:2], D.PLANAR[2])] + ([(g["own"][:2], g["own"][2])] if "own" in g else [])


@pytest.mark.parametrize("g", GEOMS, ids=[g["name"] for g in GEOMS])
def test_restatement_against_the_c_oracle(g):
    kw = {n: g[n] for n in ("k", "s", "p", "d", "groups") if n in g}
    for (H, W), B in _sizes(g):
        if min(D.out_size(H, W, kw.get("k", 3), kw.get("s", 1), kw.get("p", 1), kw.get("d", 1))) < 1:
            continue
        o = D.operands(g["C"], g["Co"], g["dg"], H, W, B, "exact", narrow=g.get("narrow", False), **kw)
        for bias in (True, False):          # with the bias and without it (the drop-in's bias_or_null)
            out, mag, _ = D.reference(o, bias=bias)
            assert torch.equal(out, _oracle(o, bias)), "exact family: the fp32 oracle and the fp64 restatement differ"
        for scale in (0.3, 4.0):
            o = D.operands(g["C"], g["Co"], g["dg"], H, W, B, "random", scale=scale, **kw)
            o["x"], o["w"], o["bias"] = (o[n].float().double() for n in ("x", "w", "bias"))
            n = (g["C"] // kw.get("groups", 1)) * kw.get("k", 3) ** 2
            for bias in (True, False):
                out, mag, _ = D.reference(o, bias=bias)
                assert bool(((out - _oracle(o, bias)).abs() <= (n + 30) * D.U * (mag + (o["bias"].abs() if bias else 0.0)) + 1e-30).all())


def test_fixed_positions_are_sampled():
    """every target of dcn_fp64.fixed_offsets IS a sampling position of the case (all 20 wherever the case has 20 slots (image, group, tap, pixel);
    on 1x1 images the limits of h, then of w, as far as the slots go), each on a slot of its own, in both families"""
    for g in GEOMS:
        kw = {n: g[n] for n in ("k", "s", "p", "d", "groups") if n in g}
        k, s, p, d = (kw.get(n, v) for n, v in (("k", 3), ("s", 1), ("p", 1), ("d", 1)))
        for (H, W), B in _sizes(g):
            Ho, Wo = D.out_size(H, W, k, s, p, d)
            if min(Ho, Wo) < 1:
                continue
            for fam in ("exact", "random"):
                o = D.operands(g["C"], g["Co"], g["dg"], H, W, B, fam, narrow=g.get("narrow", False), scale=0.3, **kw)
                pairs = D.fixed_offsets(H, W, g.get("narrow", False))
                total = B * g["dg"] * k * k * Ho * Wo
                assert len(o["planted"]) == min(total, len(pairs)) == len({q[:4] for q in o["planted"]})
                assert len(pairs) == 20 and (total < 20 or len(o["planted"]) == 20)
                hp, wp = D.positions(Ho, Wo, k, s, p, d, o["offset"])
                for (b_, g_, t_, px, th, tw) in o["planted"]:
                    assert float(hp[b_, g_, t_].reshape(-1)[px]) == float(torch.tensor(th, dtype=torch.float32)), (g["name"], H, W, th)
                    assert float(wp[b_, g_, t_].reshape(-1)[px]) == float(torch.tensor(tw, dtype=torch.float32)), (g["name"], H, W, tw)


def test_restatement_is_a_convolution_at_zero_and_integer_offsets():
    for k, s, p, d, H, W in ((3, 1, 1, 1, 5, 7), (3, 2, 2, 2, 9, 8), (1, 1, 0, 1, 4, 4)):
        o = D.operands(16, 8, 2, H, W, 2, "random", k=k, s=s, p=p, d=d)
        o["offset"].zero_()
        o["mask"], o["is_logit"] = torch.ones_like(o["mask"]), False
        out, _, _ = D.reference(o)
        want = D.conv2d_reference(o["x"], o["w"], o["bias"], k, s, p, d)
        assert float((out - want).abs().max()) < 1e-12 * float(want.abs().max())
        # one integer shift (dy, dx) for every tap, without padding (a padded position may be shifted INTO the image): the convolution of
        # the shifted, zero-filled input
        o = D.operands(16, 8, 2, H, W, 2, "random", k=k, s=s, p=0, d=d)
        o["mask"], o["is_logit"], p = torch.ones_like(o["mask"]), False, 0
        dy, dx = 1, -2
        ov = o["offset"].view(2, 2, k * k, 2, -1)
        ov[:, :, :, 0], ov[:, :, :, 1] = dy, dx
        out, _, _ = D.reference(o)
        xs = torch.zeros_like(o["x"])
        xs[:, :H - dy, max(0, -dx):] = o["x"][:, dy:, :W + dx] if dx < 0 else o["x"][:, dy:, dx:]
        want = D.conv2d_reference(xs, o["w"], o["bias"], k, s, p, d)
        assert float((out - want).abs().max()) < 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("c", D.LEAN, ids=[c["name"] for c in D.LEAN])
def test_exact_family_is_representable_and_not_empty(c):
    tile = D.tile_pixels(c["C"], c["Co"], c["dg"], c["single"])
    for (H, W), B in zip(D.SIZES, (3, 1, 3, 1, 3, 1)):
        o = D.operands(c["C"], c["Co"], c["dg"], H, W, B, "exact", narrow=c["single"])
        out, mag, smag = D.reference(o)
        unit = 8.0 if c["single"] else 64.0
        assert torch.equal(out * unit, (out * unit).round()) and float(mag.max()) <= 8 * (3 if c["single"] else 2) + 1e-9
        assert float(D.tile_sums(mag + o["bias"].abs(), tile)[0].max()) * unit < 2.0 ** 24
        assert float(smag.max()) <= (3 if c["single"] else 2)
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(o["x"].to(dt).double(), o["x"]) and torch.equal(o["w"].to(dt).double(), o["w"])
        w = o["w"]
        cpg = c["C"] // c["dg"]
        assert bool((w != 0).any(-1).any(-1).any(-1).all()), "an output channel without a filter tap"
        assert bool((w != 0).any(0).any(0).reshape(-1).all()), "a tap without a filter tap"
        assert bool((w != 0).any(0).any(-1).any(-1).view(-1, 8).any(-1).all()), "an 8-channel chunk without a filter tap"
        assert cpg in (32, 64) and int((out != 0).sum()) * 4 > out.numel()


@pytest.mark.parametrize("mu", D.MUTATIONS)
def test_mutations(mu):
    hit_exact = hit_random = 0
    for c in (D.LEAN[0], D.LEAN[2], D.LEAN[7]):
        for (H, W), B in zip(D.SIZES, (3, 1, 3, 1, 3, 3)):
            if mu == "group_of_next" and c["dg"] == 1:
                continue
            o = D.operands(c["C"], c["Co"], c["dg"], H, W, B, "exact", narrow=c["single"])
            want, _, _ = D.reference(o)
            got, _, _ = D.reference(o, mu)
            hit_exact += int(not torch.equal(got, want))
            o = D.operands(c["C"], c["Co"], c["dg"], H, W, B, "random", scale=0.3)
            want, mag, _ = D.reference(o)
            got, _, _ = D.reference(o, mu)
            sl = D.slack(o, mag, "single" if c["single"] else "split", torch.bfloat16)
            hit_random += int(bool(((got - want).abs() > sl).any()))
            if mu in D.SILENT:
                assert torch.equal(got, want)
    if mu in D.SILENT:
        assert hit_exact == 0 and hit_random == 0
    else:
        assert hit_exact >= 6 and hit_random >= 6, (mu, hit_exact, hit_random)
