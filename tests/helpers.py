import math
from fractions import Fraction

import numpy as np

# ---- shared by the exact-reference suites (tests/test_primitives_exact.py, tests/test_matrix_cores_exact.py,
#      tests/test_constraints_exact.py, tests/test_pcg_exact.py) ---------------------------------------------------------------------
U = 2.0 ** -53                                   # unit roundoff of binary64
POISON = -1.2345678912345e+77                    # (a value no operation here produces)


def gamma(k):
    """gamma_k = k u / (1 - k u): k roundings compound to a relative error of at most this (Higham, Accuracy and Stability, 3.1)."""
    return Fraction(k) * Fraction(U) / (1 - Fraction(k) * Fraction(U))


def fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).tolist())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ints(seed, shape, lim=1024):
    """Integers in [-lim, lim], about a quarter of them zero, as binary64."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-lim, lim + 1, size=shape)
    a[rng.random(size=shape) < 0.25] = 0
    return a.astype(np.float64)


def short_reals(seed, n, emin=-30, emax=30, nbits=26):
    """Both signs, binary exponents spread over [emin, emax], `nbits` significant bits: 26, so that the product of two of them is
    exact (13: of four)."""
    rng = np.random.default_rng(seed)
    mant = rng.integers(2 ** (nbits - 1), 2 ** nbits, n).astype(np.float64)
    return np.ldexp(mant * rng.choice([-1.0, 1.0], n), rng.integers(emin, emax + 1, n) - (nbits - 1))


def i64(a):
    """Integer-valued binary64 data as int64 (checked)."""
    a = np.asarray(a)
    out = a.astype(np.int64)
    assert np.array_equal(out, a)
    return out


def imatmul(A, B):
    """int64 A @ B with both operands contiguous (numpy's integer product crawls on a transposed view)."""
    return np.ascontiguousarray(A) @ np.ascontiguousarray(B)


def ulp(v):
    """The spacing of binary64 at |v| (v != 0, normal range): 2^(floor(log2 |v|) - 52)."""
    return math.ldexp(1.0, math.frexp(float(v))[1] - 53)


class DiagOpRef:
    """diag(a) as an oracle-side operator (mul! protocol) without forming n x n."""

    def __init__(self, a):
        self.a = np.asarray(a, dtype=float)

    def mul_(self, dest, v, al=None, be=None):
        if al is None:
            dest[:] = self.a * v
        else:
            dest[:] = al * (self.a * v) + be * dest
        return dest

    def adjoint(self):
        return self
