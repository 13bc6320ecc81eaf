"""CPU: the backward half of tests/dcn_fp64.py, the reference of test_gpu_dcn_bwd_edges.py.
  1. the restatement against the C oracle (oracle.c_ref.dcn_backward, fp32) on every isotropic geometry the GPU file launches -- bit for bit on the
     exact family, to fp32 noise bounded by the magnitudes on the random family;
  2. against torch AUTOGRAD of the fp64 forward with the sampling positions as leaves (dcn_fp64.forward_from_positions, itself held to the
     forward restatement) -- the only check there is for the anisotropic geometry, which the oracle's scalar arguments cannot express;
  3. against F.conv2d's gradients at zero offset and unit mask, one anisotropic geometry included;
  4. the exact family's conditions, asserted: every expected element times its denominator is an integer, every sum of magnitudes times that
     denominator is below 2^24, more than a quarter of the elements of each of the five gradients are non-zero;
  5. the launcher restated (dispatch, split geometry, XCD remap) and the planted positions;
  6. every mutation of dcn_fp64.MUTATIONS_BWD changes the exact family's expected values and exceeds slack_bwd on the random family, for
     every dispatch it applies to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dcn_fp64 as D
from oracle import c_ref

ISO = D.BWD_GEOMS[:4]
ANISO = D.BWD_GEOMS[4]
SIZES_B = list(zip(D.SIZES, (1, 3, 1, 3, 1, 3)))


def _generic(c):
    return dict(name="generic-%dx%d-g%d-dg%d" % (c[5], c[5], c[9], c[10]), C=c[1], Co=c[4], dg=c[10], groups=c[9], geom=dict(k=c[5], s=c[6], p=c[7], d=c[8]),
                own=(c[2], c[3], c[0]))


GENERIC = [_generic(c) for c in D.GENERIC]


def _ops(c, ge, H, W, B, fam, scale=None):
    return D.operands_bwd(c["C"], c["Co"], c["dg"], H, W, B, fam, k=ge["k"], s=ge["s"], p=ge["p"], d=ge["d"], groups=c.get("groups", 1), scale=scale)


def _has_output(ge, H, W):
    return min(D.out_size(H, W, ge["k"], ge["s"], ge["p"], ge["d"])) >= 1


def _oracle(o):
    k, s, p, d, dg, groups = o["geom"]
    B = o["x"].shape[0]
    Ho, Wo = D.out_size(o["x"].shape[1], o["x"].shape[2], k, s, p, d)
    r = c_ref.dcn_backward(o["x"].permute(0, 3, 1, 2).numpy(), o["offset"].view(B, -1, Ho, Wo).numpy(), o["mask"].float().view(B, -1, Ho, Wo).numpy(),
                           o["w"].numpy(), o["gout"].permute(0, 3, 1, 2).numpy(), stride=s, padding=p, dilation=d, groups=groups, dg=dg)
    gx, goff, gm, gw, gb = (torch.from_numpy(np.ascontiguousarray(a)).double() for a in r)
    return dict(gx=gx.permute(0, 2, 3, 1), goff=goff.reshape(B, -1, Ho * Wo), gmask=gm.reshape(B, -1, Ho * Wo), gw=gw, gb=gb)


def _noise(o, ref):
    """fp32 noise of ANOTHER fp32 evaluation (the oracle's own order): every chain either path counts, and 30 for the element's own arithmetic"""
    B, H, W, C = o["x"].shape
    k, s, p, d, dg, groups = o["geom"]
    Ho, Wo = D.out_size(H, W, k, s, p, d)
    n = o["w"].shape[0] // groups + C // dg + B * Ho * Wo + 30
    out = {name: (n + (ref["cnt"] if name == "gx" else 0)) * D.U * ref["mag"][name] + 1e-30 for name in D.BWD_NAMES}
    out["gx"] = out["gx"] + 4 * D.U * (max(H, W) + 1) * ref["gx_flat"]
    return out


CASES = [(c, ge) for c in D.BWD for ge in ISO] + [(c, c["geom"]) for c in GENERIC]


def _sizes(c, ge):
    out = list(SIZES_B)
    if "own" in c:
        out.append((c["own"][:2], c["own"][2]))
    elif ge["name"] == "3x3":
        out += [((h, w), b) for h, w, b in D.BWD_SPECIAL if h < 46 or c["Co"] == 128]
    return out


@pytest.mark.parametrize("c,ge", CASES, ids=["%s-%s" % (c["name"], ge.get("name", "own")) for c, ge in CASES])
def test_restatement_against_the_c_oracle(c, ge):
    for (H, W), B in _sizes(c, ge):
        if not _has_output(ge, H, W):
            continue
        o = _ops(c, ge, H, W, B, "exact")
        ref, orc = D.reference_bwd(o), _oracle(o)
        for name in D.BWD_NAMES:
            assert torch.equal(ref[name], orc[name]), "exact family, %s: the fp32 oracle and the fp64 restatement differ" % name
        if H >= 15:
            continue          # the large sizes: the exact family has compared every element
        for scale in (0.3, 4.0):
            o = _ops(c, ge, H, W, B, "random", scale)
            ref, orc = D.reference_bwd(o), _oracle(o)
            tol = _noise(o, ref)
            for name in D.BWD_NAMES:
                assert bool(((ref[name] - orc[name]).abs() <= tol[name]).all()), (name, H, W, B, scale)


def _autograd(o):
    k, s, p, d, dg, groups = o["geom"]
    B, H, W, C = o["x"].shape
    Ho, Wo = D.out_size(H, W, k, s, p, d)
    hp, wp = D.positions(Ho, Wo, k, s, p, d, o["offset"])
    x, m, w = (o[n].double().clone().requires_grad_(True) for n in ("x", "mask", "w"))
    hp, wp = hp.double().requires_grad_(True), wp.double().requires_grad_(True)
    bias = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    out = D.forward_from_positions(x, hp, wp, m, w, bias, dg, groups)
    fwd, _, _ = D.dcn_fp64(o["x"], o["offset"], o["mask"].double(), o["w"], None, k, s, p, d, dg, groups)
    assert float((out.detach() - fwd).abs().max()) <= 1e-12 * max(1.0, float(fwd.abs().max())), "forward_from_positions is not the forward restatement"
    (out * o["gout"]).sum().backward()
    K = hp.shape[2]
    goff = torch.stack((hp.grad, wp.grad), 3).reshape(B, dg * 2 * K, Ho * Wo)
    return dict(gx=x.grad, goff=goff, gmask=m.grad.view(B, dg * K, Ho * Wo), gw=w.grad, gb=bias.grad)


AUTOGRAD = [(c, ge) for c in D.BWD for ge in (D.BWD_GEOMS[0], ANISO)] + [(c, c["geom"]) for c in GENERIC] + [(GENERIC[1], ANISO)]


@pytest.mark.parametrize("c,ge", AUTOGRAD, ids=["%s-%s" % (c["name"], ge.get("name", "own")) for c, ge in AUTOGRAD])
def test_restatement_against_autograd_of_the_forward(c, ge):
    for (H, W), B in (((5, 7), 2), ((1, 9), 1), ((5, 13), 1)):
        if not _has_output(ge, H, W):
            continue
        for fam, scale in (("exact", None), ("random", 0.3), ("random", 4.0)):
            o = _ops(c, ge, H, W, B, fam, scale)
            ref, ag = D.reference_bwd(o), _autograd(o)
            for name in D.BWD_NAMES:
                assert bool(((ref[name] - ag[name]).abs() <= 1e-13 * ref["mag"][name] + 1e-300).all()), (name, H, W, fam, scale)


@pytest.mark.parametrize("ge", (D.BWD_GEOMS[0], dict(k=3, s=2, p=2, d=2), D.BWD_GEOMS[3], ANISO), ids=("3x3", "s2-d2", "1x1", "aniso"))
def test_restatement_is_the_convolutions_backward_at_zero_offset(ge):
    for groups, dg in ((1, 2), (2, 1)):
        o = D.operands_bwd(16, 8, dg, 9, 8, 2, "random", k=ge["k"], s=ge["s"], p=ge["p"], d=ge["d"], groups=groups)
        o["offset"].zero_()
        o["mask"] = torch.ones_like(o["mask"])
        ref = D.reference_bwd(o)
        x = o["x"].permute(0, 3, 1, 2).clone().requires_grad_(True)
        w = o["w"].clone().requires_grad_(True)
        b = torch.zeros(8, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, w, b, D.pair(ge["s"]), D.pair(ge["p"]), D.pair(ge["d"]), groups)
        (y * o["gout"].permute(0, 3, 1, 2)).sum().backward()
        for name, want in (("gx", x.grad.permute(0, 2, 3, 1)), ("gw", w.grad), ("gb", b.grad)):
            assert bool(((ref[name] - want).abs() <= 1e-13 * ref["mag"][name] + 1e-300).all()), name
        assert int((ref["cnt"] > 0).sum()) > 0


EXACT = [(c, ge) for c in D.BWD for ge in D.BWD_GEOMS] + [(c, c["geom"]) for c in GENERIC]


@pytest.mark.parametrize("c,ge", EXACT, ids=["%s-%s" % (c["name"], ge.get("name", "own")) for c, ge in EXACT])
def test_exact_family_is_representable_and_not_empty(c, ge):
    """every size and batch the GPU file runs the geometry on"""
    sizes = [((h, w), b) for (h, w) in D.SIZES for b in D.BS]
    if "own" in c:
        sizes.append((c["own"][:2], c["own"][2]))
    elif ge["name"] == "3x3":
        sizes += [((h, w), b) for h, w, b in D.BWD_SPECIAL if h < 15 or c["Co"] == 128]
    for (H, W), B in sizes:
        if not _has_output(ge, H, W):
            continue
        o = _ops(c, ge, H, W, B, "exact")
        for n in ("x", "w", "gout"):
            assert torch.equal(o[n], o[n].round()) and float(o[n].abs().max()) <= 2
        assert torch.equal(o["offset"] * 4, (o["offset"] * 4).round())
        assert torch.equal(o["mask"] * 4, (o["mask"] * 4).round()) and float(o["mask"].min()) >= 0.25 and not o["is_logit"]
        ref = D.reference_bwd(o)
        for name in D.BWD_NAMES:
            v, den = ref[name], D.BWD_DENOM[name]
            assert torch.equal(v * den, (v * den).round()), (name, H, W, B)
            assert float(ref["mag"][name].max()) * den < 2.0 ** 24, (name, H, W, B)
            assert float(ref["mag"][name].max()) + 0.5 < 2.0 ** 24 / den          # the 0.5 grad_weight / grad_bias are accumulated into
            assert int((v != 0).sum()) * 4 > v.numel(), (name, H, W, B, float((v != 0).double().mean()))


def test_fixed_positions_are_sampled():
    """every target of dcn_fp64.fixed_offsets is a sampling position of the random family's case (all 20 wherever it has 20 slots) and of the exact
    family's (a quarter of its slots at most), each on a slot of its own"""
    for c, ge in EXACT:
        for (H, W), B in SIZES_B:
            if not _has_output(ge, H, W):
                continue
            Ho, Wo = D.out_size(H, W, ge["k"], ge["s"], ge["p"], ge["d"])
            kh, kw = D.pair(ge["k"])
            total = B * c["dg"] * kh * kw * Ho * Wo
            for fam, share in (("exact", 4), ("random", 1)):
                o = _ops(c, ge, H, W, B, fam, 0.3)
                assert len(o["planted"]) == min(total // share, 20) == len({q[:4] for q in o["planted"]})
                hp, wp = D.positions(Ho, Wo, ge["k"], ge["s"], ge["p"], ge["d"], o["offset"])
                for (b_, g_, t_, px, th, tw) in o["planted"]:
                    assert float(hp[b_, g_, t_].reshape(-1)[px]) == float(torch.tensor(th, dtype=torch.float32)), (c["name"], H, W, th)
                    assert float(wp[b_, g_, t_].reshape(-1)[px]) == float(torch.tensor(tw, dtype=torch.float32)), (c["name"], H, W, tw)


def test_launcher_restated():
    for c in D.BWD:
        assert D.bwd_dispatch(c["C"], c["Co"], c["dg"]) == c["want"]
    assert {c["want"][1:] for c in D.BWD} == {(1, 1, 4, 2), (2, 2, 8, 1), (1, 1, 8, 2), (2, 2, 4, 1)}
    for c in GENERIC:
        assert D.bwd_dispatch(c["C"], c["Co"], c["dg"], c["groups"]) == ("generic",)
    assert D.bwd_dispatch(128, 64, 4) == ("generic",) and D.bwd_dispatch(128, 128, 4, 2) == ("generic",)          # Co = 64 has no backward instantiation
    assert D.bwd_split(1) == (64, 1, 1) and D.bwd_split(3 * 65) == (64, 1, 4) and D.bwd_split(2048) == (64, 1, 32)
    assert D.bwd_split(2049) == (128, 2, 17) and D.bwd_split(46 * 46) == (128, 2, 17)          # accumulators carried over two tiles, 15 empty splits
    for n in range(1, 40):
        tiles = [D.bwd_tile_of_block(b, n) for b in range(n)]
        assert sorted(tiles) == list(range(n))
        assert (tiles == list(range(n))) == (n <= 8)
    assert -(-3 * 15 * 15 // 64) == 11 and -(-4 * 25 // 64) == 2 and 64 // 25 == 2          # 11 tiles; a tile of 64 pixels holds images 0, 1 and part of 2


def _mutation_cases(mu):
    """(case, geometry, H, W, B) a mutation applies to, for every dispatch it applies to"""
    out = []
    for c in D.BWD + GENERIC:
        mfma = "groups" not in c
        if mu == "group_of_next" and c["dg"] == 1:
            continue
        if mu == "khkw_swapped":
            out.append((c, ANISO, 5, 13, 3))
        elif mu == "gw_past_64_missing":
            if mfma and c["Co"] == 128:          # a split holds more than one tile from 2049 pixels on; on the generic path there are no splits
                out.append((c, D.BWD_GEOMS[0], 46, 46, 1))
        elif mfma:
            out += [(c, D.BWD_GEOMS[0], 5, 7, 3), (c, D.BWD_GEOMS[0], 5, 13, 3)]
        elif not (mu == "gmask_of_next_tap" and c["geom"]["k"] == 1):
            out.append((c, c["geom"], c["own"][0], c["own"][1], max(2, c["own"][2])))
    return out


@pytest.mark.parametrize("mu", D.MUTATIONS_BWD)
def test_mutations(mu):
    cases = _mutation_cases(mu)
    assert len(cases) >= 2
    for c, ge, H, W, B in cases:
        path = "generic" if "groups" in c else "mfma"
        o = _ops(c, ge, H, W, B, "exact")
        want, got = D.reference_bwd(o), D.reference_bwd(o, mu)
        assert any(not torch.equal(want[n], got[n]) for n in D.BWD_NAMES), (mu, c["name"], "exact")
        o = _ops(c, ge, H, W, B, "random", 0.3)
        want, got = D.reference_bwd(o), D.reference_bwd(o, mu)
        sl = D.slack_bwd(o, want, path, init=0.5)
        assert any(bool(((want[n] - got[n]).abs() > sl[n]).any()) for n in D.BWD_NAMES), (mu, c["name"], "random")
