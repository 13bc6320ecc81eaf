"""The host oracle of the weight average (csrc/weight_ema.hip): the rule in fp64 and the per-element bound of ONE step of it.

The kernel receives the decay as a C `float`: d = fp32(decay) IS the decay it applies, so the oracle uses that value, exactly, as a double;
1 - d is then exact in fp64 (d is an fp32 number in [0, 1)).  On the device
    c   = fp32(1 - d)                  one rounding of a constant          c = (1 - d)(1 + e1)
    p   = fp32(c * w)                  one rounded product                 p = c w (1 + e2)
    out = fp32(d * ema + p)            one rounded fma                     out = (d ema + p)(1 + e3)          |e_i| <= U = 2^-24
(the other constant, d, is rounded before the rule is stated and carries no error against it).  To first order
    |out - (d ema + (1 - d) w)| <= U |d ema + (1 - d) w| + 2 U |(1 - d) w| <= 3 U (|d ema| + |(1 - d) w|);
the products of two and three e's add less than 4 U^2 of the same magnitude.  Results and products below 2^-126 are subnormal and round
to the spacing 2^-149 instead: at most half of it, twice.  Hence
    bound = 4 U (|d ema| + |(1 - d) w|) + 2^-149,
counted from the arithmetic, not measured.  A plain module like fp64_bounds.py; numpy only, so the CPU tests use it too."""
import numpy as np

U = 2.0 ** -24
ROUNDINGS = 4                      # three counted above, one for the second-order terms
TINY = 2.0 ** -149


def f32(v):
    """a Python number as the C `float` argument the ABI receives, back as a double"""
    return float(np.float32(v))


def rule(ema, w, decay):
    """fp64 [n]: d ema + (1 - d) w with d = fp32(decay); ema, w: arrays of fp32 values (any float dtype)."""
    d = f32(decay)
    with np.errstate(invalid="ignore", over="ignore"):
        return d * np.asarray(ema, dtype=np.float64) + (1.0 - d) * np.asarray(w, dtype=np.float64)


def bound(ema, w, decay):
    """fp64 [n]: the most one step on the device may differ from rule() per element."""
    d = f32(decay)
    with np.errstate(invalid="ignore", over="ignore"):
        return ROUNDINGS * U * (np.abs(d * np.asarray(ema, dtype=np.float64)) + np.abs((1.0 - d) * np.asarray(w, dtype=np.float64))) + TINY


def step_f32(ema, w, decay):
    """The device's arithmetic replayed on the host in fp32 numpy: fp32(1 - d), the rounded product, and d ema + p rounded ONCE (the fma: the
    sum of two fp32 products is formed in fp64, where both are exact to far below the final rounding, and rounded to fp32)."""
    d = np.float32(decay)
    c = np.float32(1.0 - float(d))
    p = (c * np.asarray(w, dtype=np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.float64(d) * np.asarray(ema, dtype=np.float64) + p.astype(np.float64)).astype(np.float32)


def classes(x):
    """int8 [n]: 0 NaN, +-1 infinite, +-2 of normal size, +-3 zero or subnormal -- by sign bit, so that +0 and -0 differ."""
    x = np.asarray(x)
    neg = np.signbit(x)
    a = np.abs(x.astype(np.float64))
    c = np.where(np.isnan(a), 0, np.where(np.isinf(a), 1, np.where(a >= 2.0 ** -126, 2, 3)))
    return np.where(np.isnan(a), 0, np.where(neg, -c, c)).astype(np.int8)
