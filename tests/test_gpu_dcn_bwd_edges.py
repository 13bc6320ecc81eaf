"""GPU: the DCN backward PER ELEMENT against the fp64 restatement of tests/dcn_fp64.py (dcn_bwd_fp64; checked on the CPU against the C oracle,
autograd of the fp64 forward and F.conv2d's gradients, its exact family proven representable and every comparison shown sensitive:
test_dcn_bwd_fp64_host.py).  Every case goes straight through glare_mdcn_backward_f32 (fp32 only: no precision fixture):
  * the four MFMA dispatches of csrc/dcn_bwd.hip -- cpg32/Co128 data<1,1> + weight<4,1,1>, cpg64/Co256 data<2,2> + weight<8,2,2>, cpg32/Co256
    data<1,1> + weight<8,1,1>, cpg64/Co128 data<2,2> + weight<4,2,2> -- restated (dcn_fp64.bwd_dispatch) and asserted: the restatement against
    the table, the library's own choice by what it does with a NULL workspace (refused on an MFMA shape, accepted on a generic one);
  * on the MFMA path 3x3, stride 2, dilation 2 with pad 2, 1x1, and one fully anisotropic geometry (kh, kw = 1, 3; sh, sw = 2, 1;
    ph, pw = 0, 1; dh, dw = 1, 2: a swap of any pair of axes changes the result);
  * three geometries of csrc/dcn_generic.hip (dcn_fp64.GENERIC: the 1x1, conv AND deformable groups, stride 2 / dilation 2 with four groups);
  * images 1x1, 1x9, 9x1, 5x7, 8x8, 5x13 (65 pixels: a full tile, a one-pixel tile, a second split), B in {1, 3}; 5x5 with B = 4 (a 64-pixel
    tile spans three images); 15x15 with B = 3 (11 tiles: the XCD remap moves tiles); 46x46 (2116 pixels: per = 128, every split holds two
    tiles, the accumulators are carried, 15 of the 32 splits are empty and must still write zeros) -- each restated and asserted.

Every launch: all five outputs sit in guarded buffers (NaN guards; grad_input / grad_offset / grad_mask NaN-filled and fully overwritten,
grad_weight / grad_bias at 0.5 and accumulated into); the workspace is NaN-filled, exactly glare_mdcn_backward_workspace_bytes long inside a
longer NaN buffer whose tail must stay NaN, and in the second run starts 4 bytes past a 256-byte boundary.  Three runs: the second has the
bits of the first in grad_offset / grad_mask / grad_weight / grad_bias (grad_input: the same bits in the exact family, bounded in the random
one -- its atomics add in any order); the third passes NULL for grad_input (stage 3: no scatter) and grad_bias and has the same bits in the
other three, the bias buffer untouched.

Offsets: the exact family, random of scale 0.3 and 4, and in every case the fixed positions of dcn_fp64.fixed_offsets: exactly -1, inside
(-1, 0), exactly H - 1, inside (H - 1, H), exactly H, the same for w, +-1e4 and +-3e9.  The last is beyond `int`; read before it was run:
an out-of-image sample forms no address that is dereferenced or scattered to.  In dcn_bwd.hip Gather::issue converts floorf(h) to int
(saturating on the device) and forms q.pix[] in 64-bit arithmetic, but `inside` is part of every ok[c]; load8b() reads only under ok
(`ok ? *p : 0`), and the scatter plan stores -1 unless valid && ok[c], which the atomics loop skips.  In dcn_generic.hip corners_at() -- the
only place y0 * W + x0 is formed -- bilinear() and coordinate_weight() are reached only under `inside`, and so is the scatter; the weight
kernel samples under the same test.

EQUAL: the exact family, all five gradients bit for bit.  BOUNDED: the random family within dcn_fp64.slack_bwd, per element.  The training
entry glare_amd.autograd.dcn (DcnFn.backward: the slicing of `om`, the sigmoid chain on grad_mask, the one bf16 rounding of gx) has one
small case.  Measured / bound on the MI355X: profiles/dcn_backward.txt."""
import pytest
import torch

import dcn_fp64 as D
import helpers_fp64 as H_
from conv_fp64 import sigmoid_rel
from fp64_bounds import U, assert_f32, assert_rounded
from glare_amd import _lib, ops
from glare_amd._lib import ptr, stream_handle

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64
INIT = 0.5
FAMILIES = (("exact", None), ("random", 0.3), ("random", 4.0))
OVERWRITTEN, ACCUMULATED = ("gx", "goff", "gmask"), ("gw", "gb")


class _Buf:
    """an output in a NaN buffer with guards; the owned region starts at `fill`"""

    def __init__(self, shape, fill):
        n = 1
        for v in shape:
            n *= v
        self.flat = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device="cuda")
        self.body = self.flat[GUARD:GUARD + n].view(shape)
        if fill == fill:
            self.body.fill_(fill)

    def guards_intact(self):
        return bool(torch.isnan(self.flat[:GUARD]).all()) and bool(torch.isnan(self.flat[-GUARD:]).all())


class _Dev:
    """one case's operands on the device in the drop-in's layouts (NCHW fp32) and its poisoned workspace"""

    def __init__(self, o):
        k, s, p, d, dg, groups = o["geom"]
        self.o, self.lib = o, _lib.main_lib()
        self.B, self.H, self.W, self.C = o["x"].shape
        self.Co, self.dg, self.groups = o["w"].shape[0], dg, groups
        self.geom = D.pair(k) + D.pair(s) + D.pair(p) + D.pair(d)
        self.Ho, self.Wo = D.out_size(self.H, self.W, k, s, p, d)
        K = self.geom[0] * self.geom[1]
        self.x = o["x"].permute(0, 3, 1, 2).float().contiguous().cuda()
        self.off = o["offset"].view(self.B, dg * 2 * K, self.Ho, self.Wo).contiguous().cuda()
        self.msk = o["mask"].float().view(self.B, dg * K, self.Ho, self.Wo).contiguous().cuda()
        self.w = o["w"].float().contiguous().cuda()
        self.gout = o["gout"].permute(0, 3, 1, 2).float().contiguous().cuda()
        for a, b in ((self.x, o["x"].permute(0, 3, 1, 2)), (self.w, o["w"]), (self.gout, o["gout"].permute(0, 3, 1, 2)), (self.msk.view(self.B, -1, self.Ho * self.Wo), o["mask"])):
            assert torch.equal(a.cpu().double(), b.double()), "an operand is not a number of fp32"
        self.need = self.lib.glare_mdcn_backward_workspace_bytes(self.B, self.C, self.H, self.W, self.Co, self.geom[0], self.geom[1])
        assert self.need == D.bwd_workspace_bytes(self.B, self.C, self.H, self.W, self.Co, self.geom[0], self.geom[1]) and self.need % 4 == 0
        self.ws = torch.empty(self.need // 4 + 256, dtype=torch.float32, device="cuda")

    def shapes(self):
        K = self.geom[0] * self.geom[1]
        return dict(gx=(self.B, self.C, self.H, self.W), goff=(self.B, self.dg * 2 * K, self.Ho, self.Wo), gmask=(self.B, self.dg * K, self.Ho, self.Wo),
                    gw=tuple(self.w.shape), gb=(self.Co,))

    def launch(self, gx=True, gb=True, unaligned=False, ws=True, nws=None, null=()):
        """-> (return code, the five buffers); the workspace is NaN-filled first and its tail checked afterwards"""
        bufs = {n: _Buf(sh, NAN if n in OVERWRITTEN else INIT) for n, sh in self.shapes().items()}
        self.ws.fill_(NAN)
        base = self.ws.data_ptr()
        assert base % 4 == 0
        skip = ((4 - base) % 256) if unaligned else ((-base) % 256)
        assert (base + skip) % 256 == (4 if unaligned else 0) and skip % 4 == 0 and skip // 4 + self.need // 4 <= self.ws.numel()
        a = dict(x=ptr(self.x), off=ptr(self.off), msk=ptr(self.msk), w=ptr(self.w), gout=ptr(self.gout), gx=ptr(bufs["gx"].body) if gx else None,
                 goff=ptr(bufs["goff"].body), gmask=ptr(bufs["gmask"].body), gw=ptr(bufs["gw"].body), gb=ptr(bufs["gb"].body) if gb else None)
        for n in null:
            a[n] = None
        rc = self.lib.glare_mdcn_backward_f32(a["x"], a["off"], a["msk"], a["w"], a["gout"], a["gx"], a["goff"], a["gmask"], a["gw"], a["gb"], self.B, self.C, self.H,
                                              self.W, self.Co, *self.geom, self.groups, self.dg, (base + skip) if ws else None,
                                              self.need if nws is None else nws, stream_handle())
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.ws[:skip // 4]).all()) and bool(torch.isnan(self.ws[skip // 4 + self.need // 4:]).all()), "written outside the workspace"
        for n, b in bufs.items():
            assert b.guards_intact(), "%s: written outside the owned region" % n
        return rc, bufs

    def untouched(self, bufs):
        return all(bool(torch.isnan(bufs[n].body).all()) for n in OVERWRITTEN) and all(bool((bufs[n].body == INIT).all()) for n in ACCUMULATED) \
            and bool(torch.isnan(self.ws).all())


def _expected(ref, dev):
    """the restatement in the drop-in's layouts, fp64; grad_weight / grad_bias on top of what the buffers held"""
    return dict(gx=ref["gx"].permute(0, 3, 1, 2).contiguous(), goff=ref["goff"].view(dev.shapes()["goff"]), gmask=ref["gmask"].view(dev.shapes()["gmask"]),
                gw=ref["gw"] + INIT, gb=ref["gb"] + INIT)


def _bounds(o, ref, dev, path):
    sl = D.slack_bwd(o, ref, path, init=INIT)
    return dict(gx=sl["gx"].permute(0, 3, 1, 2).contiguous(), goff=sl["goff"].view(dev.shapes()["goff"]), gmask=sl["gmask"].view(dev.shapes()["gmask"]), gw=sl["gw"], gb=sl["gb"])


def _case(c, ge, Hh, W, B, fam, scale, label):
    """one case through the three runs; -> nothing, asserts everything the header lists"""
    path = D.bwd_dispatch(c["C"], c["Co"], c["dg"], c.get("groups", 1))[0]
    o = D.operands_bwd(c["C"], c["Co"], c["dg"], Hh, W, B, fam, k=ge["k"], s=ge["s"], p=ge["p"], d=ge["d"], groups=c.get("groups", 1), scale=scale)
    dev = _Dev(o)
    on_dev = {n: (v.cuda() if torch.is_tensor(v) else v) for n, v in o.items()}
    ref = D.reference_bwd(on_dev)
    want = _expected(ref, dev)
    where = "%s:%dx%dx%d:%s%s" % (label, B, Hh, W, fam, scale or "")
    rc1, first = dev.launch()
    rc2, second = dev.launch(unaligned=True)
    rc3, third = dev.launch(gx=False, gb=False)
    assert (rc1, rc2, rc3) == (0, 0, 0), where
    for n in D.BWD_NAMES:
        assert not bool(torch.isnan(first[n].body).any()) and not bool(torch.isnan(second[n].body).any()), where + ": %s keeps part of its NaN fill" % n
    for n in ("goff", "gmask", "gw", "gb"):
        H_.assert_same_bits(second[n].body, first[n].body, where + ": two runs differ in " + n)
    for n in ("goff", "gmask", "gw"):
        H_.assert_same_bits(third[n].body, first[n].body, where + ": without grad_input / grad_bias, " + n)
    assert bool(torch.isnan(third["gx"].body).all()) and bool((third["gb"].body == INIT).all()), where + ": a NULL output's stand-in was written"
    if fam == "exact":
        for n in D.BWD_NAMES:
            H_.assert_same_bits(first[n].body, want[n].float(), where + " EQUAL " + n)
        H_.assert_same_bits(second["gx"].body, first["gx"].body, where + ": two runs differ in gx")
    else:
        tol = _bounds(on_dev, ref, dev, path)
        for n in D.BWD_NAMES:
            assert_f32(first[n].body, want[n], tol[n], "bwd %s %s %s%s" % (label, n, fam, scale))
        assert_f32(second["gx"].body, want["gx"], tol["gx"], "bwd %s gx %s%s" % (label, fam, scale))


def _assert_dispatch(c):
    """the restatement against the table, and the library's own choice: only the MFMA path needs (and insists on) a workspace"""
    lib = _lib.main_lib()
    groups = c.get("groups", 1)
    d = D.bwd_dispatch(c["C"], c["Co"], c["dg"], groups)
    assert d == c["want"]
    if d[0] == "mfma":          # refused at the workspace check, which only the MFMA branch has and which stands in front of every launch and every read
        z = torch.zeros(1, device="cuda")
        rc = lib.glare_mdcn_backward_f32(ptr(z), ptr(z), ptr(z), ptr(z), ptr(z), None, ptr(z), ptr(z), ptr(z), None, 1, c["C"], 1, 1, c["Co"], 3, 3, 1, 1, 1, 1, 1, 1,
                                         groups, c["dg"], None, 0, stream_handle())
        assert rc == _lib.ERR_WORKSPACE


SIZES = [((h, w), b) for (h, w) in D.SIZES for b in D.BS]


# ---- the MFMA path: every dispatch x every geometry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ge", D.BWD_GEOMS, ids=[g["name"] for g in D.BWD_GEOMS])
@pytest.mark.parametrize("c", D.BWD, ids=[c["name"] for c in D.BWD])
def test_mfma_path_per_element(c, ge):
    _assert_dispatch(c)
    ran = 0
    for (Hh, W), B in SIZES:
        if min(D.out_size(Hh, W, ge["k"], ge["s"], ge["p"], ge["d"])) < 1:
            continue
        for fam, scale in FAMILIES:
            _case(c, ge, Hh, W, B, fam, scale, c["name"])
            ran += 1
    assert ran >= 24


# ---- tiles across images, the XCD remap, carried accumulators and empty splits ----------------------------------------------------------------------
SPECIAL = [(c, sz) for c in D.BWD for sz in D.BWD_SPECIAL if sz[0] < 15 or c["Co"] == 128]


@pytest.mark.parametrize("c,sz", SPECIAL, ids=["%s-%dx%dx%d" % (c["name"], sz[2], sz[0], sz[1]) for c, sz in SPECIAL])
def test_tiles_splits_and_remap(c, sz):
    _assert_dispatch(c)
    Hh, W, B = sz
    total = B * Hh * W
    tiles = -(-total // D.DB_PIX)
    per, tiles_per_split, busy = D.bwd_split(total)
    order = [D.bwd_tile_of_block(b, tiles) for b in range(tiles)]
    if sz == (5, 5, 4):          # pixels 0 .. 63 are images 0, 1 and 14 pixels of image 2
        assert (tiles, per, busy) == (2, 64, 2) and 63 // 25 == 2 and order == [0, 1]
    elif sz == (15, 15, 3):
        assert (tiles, per, busy) == (11, 64, 11) and sorted(order) == list(range(11)) and order != list(range(11)) and 225 % 64 != 0
    else:
        assert total == 2116 > D.DB_SPLITS * D.DB_PIX and (tiles, per, tiles_per_split, busy) == (34, 128, 2, 17) and D.DB_SPLITS - busy == 15
        assert sorted(order) == list(range(34)) and order != list(range(34))
    for fam, scale in FAMILIES:
        _case(c, D.BWD_GEOMS[0], Hh, W, B, fam, scale, c["name"])


# ---- dcn_generic.hip ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", D.GENERIC, ids=("1x1", "grouped", "s2-d2-groups4"))
def test_generic_path_per_element(g):
    from test_gpu_dcn import GENERIC_CASES
    assert tuple(g) in [tuple(q) for q in GENERIC_CASES]
    c = dict(name="generic-%dx%d-g%d-dg%d" % (g[5], g[5], g[9], g[10]), C=g[1], Co=g[4], dg=g[10], groups=g[9], want=("generic",))
    ge = dict(k=g[5], s=g[6], p=g[7], d=g[8])
    _assert_dispatch(c)
    ran = 0
    for (Hh, W), B in list(zip(D.SIZES, (3, 1, 3, 1, 3, 3))) + [((g[2], g[3]), g[0])]:
        if min(D.out_size(Hh, W, ge["k"], ge["s"], ge["p"], ge["d"])) < 1:
            continue
        for fam, scale in FAMILIES:
            _case(c, ge, Hh, W, B, fam, scale, c["name"])
            ran += 1
    # a generic shape needs no workspace: NULL is accepted, and the result has the bits of the run with one
    o = D.operands_bwd(c["C"], c["Co"], c["dg"], g[2], g[3], g[0], "exact", k=ge["k"], s=ge["s"], p=ge["p"], d=ge["d"], groups=c["groups"])
    dev = _Dev(o)
    rc1, with_ws = dev.launch()
    rc2, without = dev.launch(ws=False, nws=0)
    assert (rc1, rc2) == (0, 0) and bool(torch.isnan(dev.ws).all()) and ran >= 9
    for n in D.BWD_NAMES:
        H_.assert_same_bits(without[n].body, with_ws[n].body, "generic, NULL workspace: " + n)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_workspace_alone():
    """cpg32 / Co128 on 2 x 5 x 7: a workspace one byte short or missing (GLARE_ERR_WORKSPACE), a NULL required pointer, C % dg != 0
    (GLARE_ERR_INVALID) -- every return stands in front of the first launch (dcn_bwd.hip), so the NaN-filled outputs, the 0.5 of grad_weight /
    grad_bias and the NaN-filled workspace come back as they went in."""
    c = D.BWD[0]
    o = D.operands_bwd(c["C"], c["Co"], c["dg"], 5, 7, 2, "exact")
    dev = _Dev(o)
    I, Wk = _lib.ERR_INVALID, _lib.ERR_WORKSPACE
    for want, kw in [(Wk, dict(nws=dev.need - 1)), (Wk, dict(ws=False)), (Wk, dict(nws=0))] + \
                    [(I, dict(null=(n,))) for n in ("x", "off", "msk", "w", "gout", "goff", "gmask", "gw")]:
        rc, bufs = dev.launch(**kw)
        assert rc == want, (kw, rc)
        assert dev.untouched(bufs), "a refused call wrote: %s" % (kw,)
    dev.dg = 3          # 128 % 3 != 0
    rc, bufs = dev.launch()
    assert rc == I and dev.untouched(bufs)
    assert _lib.main_lib().glare_mdcn_backward_workspace_bytes(0, 128, 5, 7, 128, 3, 3) == 0


# ---- the training entry -----------------------------------------------------------------------------------------------------------------------------------
def test_training_entry_small_case():
    """glare_amd.autograd.dcn forward and backward at C = 128, Co = 128, dg = 4, 5 x 13, B = 3, bf16 x, mask LOGITS.  DcnFn.backward slices `om` into
    offsets and logits, takes the sigmoid on the device (the kernels get mask values m32), chains grad_mask through m32 (1 - m32) in fp32, and rounds
    gx to bf16 once.  Bounds: slack_bwd, plus for everything linear in the mask the relative error of m32 (conv_fp64.sigmoid_rel) on the gradient's
    magnitudes; gom's logit half is g_mask m (1 - m): slack(g_mask) m (1 - m) + |g_mask| (|1 - 2 m| m rel(m) + 3 U m (1 - m)) -- the error of m32
    through the derivative, then g * y, 1 - y and their product."""
    from glare_amd import autograd as A
    B, Hh, W, C, Co, dg = 3, 5, 13, 128, 128, 4
    with ops.use_precision("bf16"):
        o = D.operands(C, Co, dg, Hh, W, B, "random", scale=0.3)
        gen = torch.Generator().manual_seed(5)
        gout = torch.randn(B, Hh, W, Co, generator=gen).float()
        x16 = o["x"].to(torch.bfloat16)
        om = torch.cat((o["offset"], o["mask"]), 1).view(B, 3 * dg * 9, Hh, W).permute(0, 2, 3, 1).contiguous()          # NHWC: offsets | logits
        ref_o = dict(o, x=x16.double().cuda(), offset=o["offset"].cuda(), mask=torch.sigmoid(o["mask"].double()).cuda(), w=o["w"].float().double().cuda(),
                     gout=gout.double().cuda(), is_logit=False)
        ref = D.reference_bwd(ref_o)
        sl = D.slack_bwd(ref_o, ref, "mfma")
        a = o["mask"].double().cuda()
        m = torch.sigmoid(a)
        rel = sigmoid_rel(a)
        rel_max = float(rel.max())

        def run(x_grad):
            x = x16.cuda().requires_grad_(x_grad)
            omd = om.cuda().requires_grad_(True)
            w = o["w"].float().cuda().requires_grad_(True)
            b = o["bias"].float().cuda().requires_grad_(True)
            out = A.dcn(x, omd, w, b, dg, 1)
            assert out.dtype == torch.float32 and out.shape == (B, Hh, W, Co)
            out.backward(gout.cuda())
            return x.grad, omd.grad, w.grad, b.grad
        gx, gom, gw, gb = run(True)
        gx0, gom0, gw0, gb0 = run(False)
        assert gx0 is None
        for got, same, n in ((gom, gom0, "gom"), (gw, gw0, "gw"), (gb, gb0, "gb")):
            H_.assert_same_bits(same, got, "entry: x.requires_grad = False changes " + n)
        assert gom.dtype == torch.float32 and gom.shape == (B, Hh, W, 3 * dg * 9) and gx.dtype == torch.bfloat16
        planar = gom.permute(0, 3, 1, 2).reshape(B, 3 * dg * 9, Hh * W).contiguous()
        n_off = 2 * dg * 9
        assert_f32(planar[:, :n_off].contiguous(), ref["goff"], sl["goff"] + rel_max * ref["mag"]["goff"], "bwd entry goff")
        chain = m * (1 - m)
        want = ref["gmask"] * chain
        tol = sl["gmask"] * chain + ref["gmask"].abs() * ((1 - 2 * m).abs() * m * rel + 3 * U * chain) + U * want.abs() + 2.0 ** -149
        assert_f32(planar[:, n_off:].contiguous(), want, tol, "bwd entry gom-logits")
        assert_rounded(gx, ref["gx"], sl["gx"] + rel_max * ref["mag"]["gx"], "bwd entry gx")
        assert_f32(gw, ref["gw"], sl["gw"] + rel_max * ref["mag"]["gw"], "bwd entry gw")
        assert_f32(gb, ref["gb"], sl["gb"], "bwd entry gb")
