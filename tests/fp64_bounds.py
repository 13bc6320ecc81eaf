"""Format helpers of the per-element fp64 tests (test_gpu_streaming_edges.py, test_gpu_backward_edges.py): the ulp of the 16-bit
format in use and the two forms of the derived bound,
    16-bit output   |got - exact| <= 0.5 ulp16(exact) + slack
    fp32 output     |got - exact| <= tol
with slack / tol the fp32 evaluation error of the kernel's own expression, counted from its source by the caller
(U = 2^-24, the relative error of ONE fp32 rounding).  Every bound goes through tolerances.within(measured / bound, 1.0), whose
table of measured values lists how much of it is used.  A plain module like tolerances.py."""
import torch

from glare_amd import ops
from tolerances import within

U = 2.0 ** -24            # one fp32 rounding, relative (half an ulp)


def _fmt():
    """(mantissa bits m, smallest normal exponent) of the 16-bit format in use."""
    return (7, -126) if ops.act_dtype() == torch.bfloat16 else (10, -14)


def _r16(x):
    return x.to(ops.act_dtype())


def _floor_log2(v):
    e = torch.floor(torch.log2(v))
    e = torch.where(torch.exp2(e) > v, e - 1, e)          # log2 may round across an exact power of two
    return torch.where(torch.exp2(e + 1) <= v, e + 1, e)


def ulp16(v):
    """2^(floor(log2 |v|) - m), the exponent floored at the format's smallest normal one (subnormals are evenly spaced)."""
    m, emin = _fmt()
    v = v.double().abs().clamp_min(2.0 ** emin)
    return torch.exp2(_floor_log2(v).clamp_min(emin) - m)


def _tag(tag):
    return "%s:%s" % (ops.precision(), tag)


def assert_rounded(got16, exact64, slack64, tag):
    """per element: |got - exact| <= 0.5 ulp16(exact) + slack"""
    assert got16.dtype == ops.act_dtype() and got16.shape == exact64.shape, (got16.dtype, got16.shape, exact64.shape)
    err = (got16.double() - exact64).abs()
    return within(float((err / (0.5 * ulp16(exact64) + slack64)).max()), 1.0, _tag(tag))


def assert_f32(got32, exact64, tol64, tag):
    """an fp32 result: |got - exact| <= tol, tol = (roundings counted in the kernel) * U * (magnitudes of the terms)"""
    assert got32.dtype == torch.float32 and got32.shape == exact64.shape, (got32.dtype, got32.shape, exact64.shape)
    return within(float(((got32.double() - exact64).abs() / tol64).max()), 1.0, _tag(tag))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _f32(v):
    """a Python number as the C `float` argument the ABI receives, back as a double"""
    return float(torch.tensor(v, dtype=torch.float32))
