"""attention_kv512 (attn_kv_fwd_kernel, d = 512) at the smallest shapes where its tile loop, its masking and its store tail can go wrong:
one tile, odd and even tile counts, a partial last key tile, a partial last query block, key splits, the hi / lo pair output and an
output pitch above 512 -- per element against an fp64 softmax computed here, under the bound tests/test_gpu_kernels.py applies to this
kernel.  Every case runs twice into a sentinel-filled buffer: the two results are identical, and nothing outside [B*N rows] x [512
channels] is written."""
import math

import pytest
import torch

from glare_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B7B          # int16 pattern of every element the kernel must not write
TAIL_ROWS = 5              # rows of the buffer beyond the B * N the kernel owns
_REF = {}


def _case(precision, B, N):
    """(q, x, fp64 reference) of one shape: computed once, shared by every launch form of that shape, never modified."""
    key = (precision, B, N)
    if key not in _REF:
        dt = torch.float16 if precision == "fp16" else torch.bfloat16
        g = torch.Generator().manual_seed(1000 * B + N)
        q = (torch.randn(B, N, 512, generator=g) * 0.15).to(dt)
        x = (torch.randn(B, N, 512, generator=g) + torch.linspace(-1, 1, 512)).to(dt)      # per-channel offsets: d is not symmetric
        s = torch.einsum("bid,bjd->bij", q.double(), x.double())                            # scale folded into q, log2 domain
        ref = torch.einsum("bij,bjd->bid", torch.softmax(s * math.log(2.0), dim=2), x.double())
        _REF[key] = (q.cuda(), x.cuda(), ref)
    return _REF[key]


def _launch(q, x, B, N, ks, pair, pitch):
    buf = torch.full((B * N + TAIL_ROWS, pitch), SENTINEL, dtype=torch.int16, device="cuda").view(q.dtype)
    out = ops.attention_kv512(q, x, N, out=buf[:B * N].view(B, N, pitch), key_splits=ks, pair=pair)
    torch.cuda.synchronize()
    lo = out._lo[..., :512].clone() if pair else None
    return buf, lo


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 63, 65, 127, 128, 129, 161])
def test_kv512_edges_match_fp64_softmax_and_write_only_their_rows(N, precision):
    n_tiles = (N + 31) // 32
    with ops.use_precision(precision):
        for B in (1, 3):
            q, x, ref = _case(precision, B, N)
            atol = 2 ** -7 * float(ref.abs().max())
            for ks in (1, 2, 3):
                if ks > n_tiles:                       # every split owns at least one key tile
                    continue
                for pair in (False, True):
                    for pitch in (512, 576):
                        tag = "%s B%d N%d ks%d pair%d pitch%d" % (precision, B, N, ks, pair, pitch)
                        buf, lo = _launch(q, x, B, N, ks, pair, pitch)
                        buf2, lo2 = _launch(q, x, B, N, ks, pair, pitch)
                        raw = buf.view(torch.int16)
                        assert torch.equal(raw, buf2.view(torch.int16)), tag + ": two runs differ"
                        assert bool((raw[B * N:] == SENTINEL).all()), tag + ": rows beyond B*N written"
                        assert bool((raw[:, 512:] == SENTINEL).all()), tag + ": bytes beyond the 512 channels written"
                        got = buf[:B * N, :512].reshape(B, N, 512).double().cpu()
                        err = (got - ref).abs()
                        print("%s: max |err| %.3e (atol %.3e)" % (tag, float(err.max()), atol))
                        assert bool((err <= atol + 2 ** -6 * ref.abs()).all()), tag
                        if pair:
                            assert torch.equal(lo.view(torch.int16), lo2.view(torch.int16)), tag + ": two runs differ (lo)"
                            both = got + lo.double().cpu()
                            assert bool(((both - ref).abs() <= atol + 2 ** -6 * ref.abs()).all()), tag + " (hi + lo)"
