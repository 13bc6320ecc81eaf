"""GPU: the forward attention OUTPUT per element against the fp64 restatement of tests/attn_fp64.py (checked on the CPU against
torch.softmax, with the exact family proven exact under a replay of the kernels' order of operations and every comparison shown sensitive:
test_attn_fp64_host.py), in both 16-bit formats: attn_fwd_kernel behind ops.attention_d512 (with and without lse=: the same bits),
attn_kv_fwd_kernel behind ops.attention_kv512 (plain and PAIR), attn_combine_kernel behind both at 2..4 key splits (its pair output too).

Shapes N in {1, 31, 32, 33, 64, 65, 127, 128, 129, 161} x B in {1, 3}; every key split 1..4 whose splits own a tile each; output pitch 512
and 576, and 516 at one split (8-byte stores on the ldo % 4 rule); plain operands and q | k (q | x) inside one wider record.

Every output lives in the middle of a flat buffer filled with the int16 pattern 0x7B7B: GUARD elements in front and behind, TAIL rows after
the B N rows the launch owns, the channels from 512 to the pitch.  Every launch runs twice into fresh buffers: the same bits.  Poison, within
the kernels' contract as read from attn.hip: rows past B N of the q / k / x allocations and the record channels outside the 512 used hold
NaN (key rows past N of the last image are cut by the buffer descriptor, `(N - 1) ldk + 512` elements per image; query rows past N read
row 0 instead); columns N .. v_pitch - 1 of V^T hold the LARGEST FINITE number of the format -- the pad that ops.conv2d(plane_pitch=) and
train_ops.transpose leave is cleared and finite, so a masked key's p = 2^-inf = 0 makes them contribute exactly 0 -- at the smallest
v_pitch (N rounded up to 32) and a larger one.

Two kinds of assertion (fp64_bounds.py):
  EQUAL    the exact family of attn_fp64.exact_case: the whole buffer, sentinel included, is the fp64 value rounded once, the pair's lo included
  BOUNDED  the random family (base-2 logits of standard deviation 4, per-channel offsets on V, three structured rows):
           |got - exact| <= 0.5 ulp16(exact) + attn_fp64's slack; the pair's hi + lo as an fp32-class value within the slack alone
Measured / bound on the MI355X: profiles/attention_dcn_forward.txt."""
import pytest
import torch

import attn_fp64 as A
import helpers_fp64 as H
from fp64_bounds import _bits, _tag, assert_rounded
from glare_amd import _lib, ops
from glare_amd._lib import ptr, stream_handle
from tolerances import within

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD, TAIL = 64, 5
REC, Q_OFF, K_OFF = 1088, 0, 576          # the strided form: q | 64 NaN channels | k (or x) in one record
PITCHES = (512, 576)
_CASES = {}


@pytest.fixture(params=("bf16", "fp16"))
def prec(request):
    with ops.use_precision(request.param):
        yield request.param


# ---- operands, built once per (format, form, family, B, N) and never modified -------------------------------------------------------------
def _rows(vals, pitch, off):
    """[B, N, 512] -> a NaN-filled [B N + TAIL, pitch] device buffer holding them at channel `off`, and the [B, N, 512] view of them"""
    B, N, _ = vals.shape
    buf = torch.full((B * N + TAIL, pitch), NAN, dtype=ops.act_dtype())
    buf[:B * N, off:off + A.HD] = vals.reshape(B * N, A.HD).to(ops.act_dtype())
    buf = buf.cuda()
    return buf, buf[:B * N].view(B, N, pitch)[..., off:off + A.HD]


def _case(form, fam, B, N):
    key = (ops.precision(), form, fam, B, N)
    if key not in _CASES:
        dt = ops.act_dtype()
        q, k, v = A.exact_case(B, N, form) if fam == "exact" else A.random_case(B, N, form, dt)
        for t in (q, k, v):
            assert torch.equal(t.to(dt).double(), t), "operands are not numbers of the format"
        c = {"B": B, "N": N}
        c["plain"] = (_rows(q, A.HD, 0)[1], _rows(k, A.HD, 0)[1], A.HD)
        rec = torch.full((B * N + TAIL, REC), NAN, dtype=dt)
        rec[:B * N, Q_OFF:Q_OFF + A.HD], rec[:B * N, K_OFF:K_OFF + A.HD] = q.reshape(-1, A.HD).to(dt), k.reshape(-1, A.HD).to(dt)
        rec = rec.cuda()
        view = rec[:B * N].view(B, N, REC)
        c["strided"] = (view[..., Q_OFF:Q_OFF + A.HD], view[..., K_OFF:K_OFF + A.HD], REC)
        if form == "d512":
            c["v_t"] = []
            for pitch in (A.tiles(N) * A.BN, A.tiles(N) * A.BN + 40):
                v_t = torch.full((B, A.HD, pitch), torch.finfo(dt).max, dtype=dt)
                v_t[:, :, :N] = v.transpose(1, 2).to(dt)
                c["v_t"].append(v_t.cuda())
        qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
        if fam == "exact":
            c["exact"] = A.attention_fp64(qd, kd, vd)
        else:
            c["exact"], c["slack"], _ = A.slack_terms(qd, kd, vd, dt)
        c["hi"] = c["exact"].to(dt)
        c["lo"] = (c["exact"] - c["hi"].double()).to(dt)
        _CASES[key] = c
    return _CASES[key]


class _Out:
    """B N + TAIL rows of `pitch` in the middle of a flat sentinel-filled buffer; `view` is what the launch gets"""

    def __init__(self, B, N, pitch):
        self.B, self.N, self.pitch = B, N, pitch
        n = (B * N + TAIL) * pitch
        self.flat = H.sentinel16((n + 2 * GUARD,), ops.act_dtype(), "cuda")
        self.view = self.flat[GUARD:GUARD + B * N * pitch].view(B, N, pitch)

    def expected(self, values):
        e = H.sentinel16((self.flat.numel(),), ops.act_dtype(), "cuda")
        e[GUARD:GUARD + self.B * self.N * self.pitch].view(self.B, self.N, self.pitch)[..., :A.HD] = values
        return e

    def owned(self):
        return self.view[..., :A.HD]


def _twice(launch):
    first, second = launch(), launch()
    for a, b in zip(first, second):
        assert torch.equal(_bits(a.flat), _bits(b.flat)), "two runs of one launch differ"
    return first


def _check(c, fam, outs, ks, tag):
    """outs: (hi,) or (hi, lo)"""
    hi = outs[0]
    if fam == "exact":
        H.assert_same_bits(hi.flat, hi.expected(c["hi"]), tag + " EQUAL")
        if len(outs) == 2:
            H.assert_same_bits(outs[1].flat, outs[1].expected(c["lo"]), tag + " EQUAL lo")
        return
    dt = ops.act_dtype()
    slack = c["slack"](ks)
    got = hi.owned().contiguous()
    H.assert_same_bits(hi.flat, hi.expected(got), tag + " outside the owned region")
    assert_rounded(got, c["exact"], slack + A.binade_extra(c["exact"], slack, dt), tag)
    if len(outs) == 2:
        lo = outs[1].owned().contiguous()
        H.assert_same_bits(outs[1].flat, outs[1].expected(lo), tag + " outside the owned region (lo)")
        # hi + lo in fp64: the compiler contracts `o * inv - hi` into one fma, so lo may hold bits below the fp32 grid of o * inv and the sum
        # need not be an fp32 number -- assert_f32's rule on the fp64 sum
        ratio = ((got.double() + lo.double() - c["exact"]).abs() / (slack + A.pair_slack(c["exact"], slack, dt))).max()
        within(float(ratio), 1.0, _tag(tag + ":hi+lo"))


def _pitches(ks):
    return PITCHES + ((516,) if ks == 1 else ())


# ---- attn_fwd_kernel (+ attn_combine_kernel) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", A.BS)
@pytest.mark.parametrize("N", A.NS)
def test_d512_output_per_element(prec, N, B):
    for fam in ("exact", "random"):
        c = _case("d512", fam, B, N)
        for ks in A.splits_of(N):
            for pitch in _pitches(ks):
                for layout in ("plain", "strided"):
                    q, k, ld = c[layout]
                    for iv, v_t in enumerate(c["v_t"]):
                        tag = "d512:%s:%dx%d:ks%d:ldo%d:%s:vp%d" % (fam, B, N, ks, pitch, layout, v_t.shape[2])

                        def launch(lse=None):
                            out = _Out(B, N, pitch)
                            r = ops.attention_d512(q, k, v_t, N, ldq=ld, ldk=ld, out=out.view, key_splits=ks, lse=lse)
                            assert r is out.view
                            return (out,)
                        outs = _twice(launch)
                        _check(c, fam, outs, ks, tag)
                        if iv == 0:          # with lse=: the other entry point, the same bits
                            lse = torch.full((B, N), NAN, dtype=torch.float32, device="cuda")
                            with_lse = launch(lse)
                            assert torch.equal(_bits(with_lse[0].flat), _bits(outs[0].flat)), tag + ": lse= changes the output"
                            assert bool(torch.isfinite(lse).all())


# ---- attn_kv_fwd_kernel<false / true> (+ attn_combine_kernel, which writes the pair at ks > 1) ---------------------------------------------
def _kv_pair(q, x, ld, B, N, ks, pitch):
    """glare_attention_kv512_pair_bf16 on sentinel-filled hi AND lo (ops.attention_kv512(pair=True) allocates lo itself)"""
    lib = _lib.lib()
    hi, lo = _Out(B, N, pitch), _Out(B, N, pitch)
    nws = lib.glare_attention_d512_splitk_workspace_bytes(B, N, ks)
    ws = torch.empty(max(int(nws), 16), dtype=torch.uint8, device="cuda") if ks > 1 else None
    _lib.check(lib.glare_attention_kv512_pair_bf16(ptr(q), ld, ptr(x), ld, ptr(hi.view), ptr(lo.view), pitch, B, N, ks, ptr(ws), nws if ks > 1 else 0,
                                                   stream_handle()), "glare_attention_kv512_pair_bf16")
    return hi, lo


@pytest.mark.parametrize("B", A.BS)
@pytest.mark.parametrize("N", A.NS)
def test_kv512_output_per_element(prec, N, B):
    for fam in ("exact", "random"):
        c = _case("kv", fam, B, N)
        for ks in A.splits_of(N):
            for pitch in _pitches(ks):
                for layout in ("plain", "strided"):
                    q, x, ld = c[layout]
                    tag = "kv512:%s:%dx%d:ks%d:ldo%d:%s" % (fam, B, N, ks, pitch, layout)

                    def launch():
                        out = _Out(B, N, pitch)
                        assert ops.attention_kv512(q, x, N, ldq=ld, ldkv=ld, out=out.view, key_splits=ks) is out.view
                        return (out,)
                    plain = _twice(launch)
                    _check(c, fam, plain, ks, tag)
                    pair = _twice(lambda: _kv_pair(q, x, ld, B, N, ks, pitch))
                    _check(c, fam, pair, ks, tag + ":pair")
                    assert torch.equal(_bits(pair[0].flat), _bits(plain[0].flat)), tag + ": the pair's hi is not the plain output"
                    if layout == "plain" and pitch == 512:          # the wrapper's own pair path: the same bits
                        r = ops.attention_kv512(q, x, N, ldq=ld, ldkv=ld, key_splits=ks, pair=True)
                        assert torch.equal(_bits(r), _bits(pair[0].owned())) and torch.equal(_bits(r._lo), _bits(pair[1].owned()))


# ---- refusals: the status, and an output nobody touched ------------------------------------------------------------------------------------
def test_refusals_leave_the_output_alone(prec):
    """every early return of attn_launch, glare_attention_kv512_pair_bf16 and glare_attention_d512_lse_bf16.  All of them stand in front of
    the launch (attn.hip: the size limits, `32-bit DMA offsets per image`, directly behind the argument checks), so the huge ldk / v_pitch /
    B of the size-limit cases never reach a kernel: the buffers stay small."""
    lib = _lib.lib()
    dt = ops.act_dtype()
    B, N, ks = 2, 33, 2
    q = torch.zeros(B * N, 512, dtype=dt, device="cuda")
    v_t = torch.zeros(B, 512, 64, dtype=dt, device="cuda")
    nws = lib.glare_attention_d512_splitk_workspace_bytes(B, N, 4)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    need = lib.glare_attention_d512_splitk_workspace_bytes(B, N, ks)
    assert lib.glare_attention_d512_splitk_workspace_bytes(B, N, 1) == 0 == lib.glare_attention_d512_splitk_workspace_bytes(0, N, 2)
    assert need == B * ks * N * 514 * 4
    out = H.sentinel16((B * N, 576), dt, "cuda")
    lse = torch.full((B, N), NAN, dtype=torch.float32, device="cuda")
    I, U_, W = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    base = dict(q=ptr(q), ldq=512, k=ptr(q), ldk=512, v=ptr(v_t), vp=64, out=ptr(out), ldo=576, B=B, N=N, ks=ks, ws=ptr(ws), nws=need)
    d512 = [(I, dict(q=None)), (I, dict(k=None)), (I, dict(v=None)), (I, dict(out=None)), (I, dict(B=0)), (I, dict(N=0)), (I, dict(ks=0)),
            (I, dict(ks=3)),                                             # 33 keys are 2 tiles: a third split would own none
            (U_, dict(ldk=1 << 25)), (U_, dict(vp=1 << 21)),             # 32-bit DMA offsets per image
            (W, dict(ldo=516)), (W, dict(ws=None)), (W, dict(nws=need - 1)),
            (U_, dict(ldq=516)), (U_, dict(ldk=516)), (U_, dict(ldo=514, ks=1)), (U_, dict(vp=68)), (U_, dict(ldq=504)), (U_, dict(ldk=504)),
            (U_, dict(ldo=508, ks=1)),
            (I, dict(vp=32)),                                            # tiles read whole 32-key groups
            (I, dict(B=(1 << 30) + 1, N=129, vp=160, ks=1))]             # 2 query blocks per image: more than 2^31 - 1 workgroups
    for want, change in d512:
        a = dict(base, **change)
        got = lib.glare_attention_d512_splitk_bf16(a["q"], a["ldq"], a["k"], a["ldk"], a["v"], a["vp"], a["out"], a["ldo"], a["B"], a["N"], a["ks"],
                                                   a["ws"], a["nws"], stream_handle())
        assert got == want, ("d512", change, got, want)
        got = lib.glare_attention_d512_lse_bf16(a["q"], a["ldq"], a["k"], a["ldk"], a["v"], a["vp"], a["out"], a["ldo"], ptr(lse), a["B"], a["N"],
                                                a["ks"], a["ws"], a["nws"], stream_handle())
        assert got == want, ("d512 lse", change, got, want)
    a = base
    assert lib.glare_attention_d512_lse_bf16(a["q"], 512, a["k"], 512, a["v"], 64, a["out"], 576, None, B, N, ks, a["ws"], need, stream_handle()) == I
    assert lib.glare_attention_d512_bf16(a["q"], 516, a["k"], 512, a["v"], 64, a["out"], 576, B, N, stream_handle()) == U_
    out_lo = H.sentinel16((B * N, 576), dt, "cuda")
    kv = [(w, ch) for w, ch in d512 if not ({"v", "vp"} & set(ch)) or "B" in ch]
    assert len(kv) == len(d512) - 4
    for want, change in kv:
        a = dict(base, **change)
        for lo in (None, ptr(out_lo)):
            got = lib.glare_attention_kv512_pair_bf16(a["q"], a["ldq"], a["k"], a["ldk"], a["out"], lo, a["ldo"], a["B"], a["N"], a["ks"], a["ws"],
                                                      a["nws"], stream_handle())
            assert got == want, ("kv512", change, got, want)
        got = lib.glare_attention_kv512_bf16(a["q"], a["ldq"], a["k"], a["ldk"], a["out"], a["ldo"], a["B"], a["N"], a["ks"], a["ws"], a["nws"],
                                             stream_handle())
        assert got == want, ("kv512 plain", change, got, want)
    torch.cuda.synchronize()
    for t in (out, out_lo):
        H.assert_same_bits(t, H.sentinel16(t.shape, dt, "cuda"), "a refused launch wrote its output")
    assert bool(torch.isnan(lse).all())
