"""The vector primitives (vec_kernel + reduce_rows_kernel, the GEMV pair: csrc/kernels.h, csrc/primitives.hip) against exactly
rounded references.

Every reference is computed on the host with the standard library only: `fractions.Fraction` (exact rationals; `float(Fraction)`
rounds correctly, once), `math.fsum` (the correctly rounded sum of its arguments) and `decimal` at 60 digits for the square roots.
numpy generates and stores the data and forms elementwise products that are exact by construction (integers, or factors of at
most 26 significant bits); its sums and matrix products are never a reference here.

  (a) integer-valued data: every product and every partial sum in any order is an integer below 2^53, so the result does not
      depend on the summation order and the assertion is ==;
  (b) the same at lengths that reach the four-way unrolled second stage and more than one tile per block, and with the grid
      capped by LFPSQP_VEC_BLOCKS;
  (c) hostile real data (cancelling sums) against the a-priori bound gamma_k * sum |terms| for summation in an arbitrary order;
  (d) the elementwise maps entry by entry, aliasing, the beta == 0 / b == 0 / a == 0 branches, "untouched beyond the range";
  (e) lfpsqp_separable against a 60-digit statement of its definition, to a RELATIVE bound.

Each case runs on the CPU emulator build and, under -m gpu, on the MI355X, with the same assertions."""
import ctypes as C
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest

import lfpsqp_jl_amd as L
from lfpsqp_jl_amd.device import nrm2_head
from lfpsqp_jl_amd.inequality import StackedVector
from tests.helpers import POISON, U, bits, fsum, gamma, ints, short_reals

SIZES = [1, 2, 3, 511, 512, 513, 1023, 1025, 2047, 2048, 2049, 4097]
GEMV_M = [1, 3, 4, 5, 96, 97, 128, 132, 133, 257]
GEMV_N = [1, 3, 1023, 1025, 2049, 4100]
BIG = 2.0 ** 20                                  # the sentinel
TILE = 512                                       # rows per vec_kernel tile (kSlabRows)


def rnd(q):
    """The binary64 value nearest to the rational q (one rounding)."""
    return float(q)


def fma(a, b, c):
    return rnd(Fraction(a) * Fraction(b) + Fraction(c))


def counts_of(n):
    """0, 1, n - 1, n and odd and even counts in between."""
    h = n // 2
    return sorted({c for c in (0, 1, n - 1, n, h | 1, h & ~1, (h | 1) + 2) if 0 <= c <= n})


def positions_of(n, count):
    return sorted({p for p in (0, count - 1, count, n - 1, 511, 512, 513, 2047, 2048, 2049) if 0 <= p < n})


def reals(seed, n, emin=-30, emax=30):
    """Full 53-bit mantissas, both signs, binary exponents spread over [emin, emax]."""
    rng = np.random.default_rng(seed)
    return np.ldexp(rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n), rng.integers(emin, emax + 1, n))


# ---- thin wrappers over the entry points that the object layer does not expose -------------------------------------------------
def dot_head(x, y, count):
    out = C.c_double()
    x.ctx.check(x.ctx.L.lfpsqp_dot_head(x.ctx.h, x.h, y.h, int(count), C.byref(out)))
    return out.value


def sumsq_shift(x, count, c):
    out = C.c_double()
    x.ctx.check(x.ctx.L.lfpsqp_sumsq_shift(x.ctx.h, x.h, int(count), float(c), C.byref(out)))
    return out.value


def affine_head(a, x, c, count, y):
    x.ctx.check(x.ctx.L.lfpsqp_affine_head(x.ctx.h, float(a), x.h, float(c), int(count), y.h))


def fill_range(v, offset, count, value):
    v.ctx.check(v.ctx.L.lfpsqp_vec_fill_range(v.ctx.h, v.h, int(offset), int(count), float(value)))


def separable(kind, mode, a, c, x, count, out=None):
    """a, c: a device vector or a float (the constants a0, c0)."""
    s = C.c_double()
    av, cv = isinstance(a, L.DeviceVector), isinstance(c, L.DeviceVector)
    x.ctx.check(x.ctx.L.lfpsqp_separable(x.ctx.h, kind, mode, a.h if av else None, 0.0 if av else float(a), c.h if cv else None,
                                         0.0 if cv else float(c), x.h, int(count), out.h if out is not None else None, C.byref(s)))
    return s.value


# ================================================================================================================================
# (a) exact equality on integer-valued data
# ================================================================================================================================
def _check_integer_reductions(ctx, n, seed=0):
    xh, yh = ints(seed + 1, n), ints(seed + 2, n)
    th, ah, ch = ints(seed + 3, n, 8), np.abs(ints(seed + 4, n, 3)) + 1.0, ints(seed + 5, n, 100)
    x, y, a, c = ctx.vector(n, xh), ctx.vector(n, yh), ctx.vector(n, ah), ctx.vector(n, ch)
    xs, x0 = ctx.vector(n, ch + th), ctx.vector(n, th)
    assert L.dot(x, y) == fsum(xh * yh)
    assert L.dot(x, x) == fsum(xh * xh)
    assert L.nrm2(x) == math.sqrt(fsum(xh * xh))                       # (sqrt of an exact integer: correctly rounded on both sides)
    assert L.amax(x) == max(abs(v) for v in xh.tolist())
    for count in counts_of(n):
        assert dot_head(x, y, count) == fsum(xh[:count] * yh[:count])
        assert nrm2_head(x, count) == math.sqrt(fsum(xh[:count] * xh[:count]))
        for cc in (0.0, 3.0, -7.0):
            assert sumsq_shift(x, count, cc) == fsum((xh[:count] - cc) ** 2)
        t = th[:count]
        # kind 0: a t^2, kind 1: a t^4 + t^2 -- per-variable (a, c) and constants (a0, c0)
        assert separable(0, 0, a, c, xs, count) == fsum(ah[:count] * t * t)
        assert separable(1, 0, a, c, xs, count) == fsum(ah[:count] * t ** 4 + t * t)
        assert separable(0, 0, 3.0, -2.0, xs, count) == fsum(3.0 * (ch[:count] + t + 2.0) ** 2)
        assert separable(1, 0, 2.0, 5.0, x0, count) == fsum(2.0 * (t - 5.0) ** 4 + (t - 5.0) ** 2)
    for v in (x, y, a, c, xs, x0):
        v.free()


@pytest.mark.parametrize("n", SIZES)
def test_reductions_are_exact_on_integer_data(dev_ctx, n):
    """dot, dot_head, nrm2, nrm2_head, sumsq_shift, amax, separable mode 0 (kinds 0 and 1): == the exact value for every count."""
    _check_integer_reductions(dev_ctx, n)


@pytest.mark.parametrize("n", SIZES)
def test_a_single_large_entry_counts_exactly_where_it_should(dev_ctx, n):
    """All zeros but one 2^20: at index 0, count - 1, count, n - 1 and around the tile edges.  An entry at index >= count must not
    reach a count-limited result (the lane pair (count - 1, count) of an odd count is where it would)."""
    ctx = dev_ctx
    threes = ctx.vector(n, np.full(n, 3.0))
    x = ctx.vector(n)
    for count in counts_of(n):
        for p in positions_of(n, count):
            xp = -BIG if p % 2 else BIG
            x.upload(np.array([xp]), p)
            inside = p < count
            assert dot_head(x, threes, count) == (3.0 * xp if inside else 0.0)
            assert dot_head(threes, x, count) == (3.0 * xp if inside else 0.0)
            assert nrm2_head(x, count) == (BIG if inside else 0.0)
            assert sumsq_shift(x, count, 0.0) == (BIG * BIG if inside else 0.0)
            assert sumsq_shift(x, count, 1.0) == float(count) + ((BIG * BIG - 2.0 * xp) if inside else 0.0)
            assert separable(0, 0, 1.0, 0.0, x, count) == (BIG * BIG if inside else 0.0)
            assert separable(1, 0, 0.0, 0.0, x, count) == (BIG * BIG if inside else 0.0)
            assert L.dot(x, threes) == 3.0 * xp and L.nrm2(x) == BIG and L.amax(x) == BIG
            x.upload(np.array([0.0]), p)
    threes.free(); x.free()


def _gemv_case(ctx, n, m, seed):
    Mh = np.asfortranarray(ints(seed, (n, m)))
    vh, th, yh = ints(seed + 1, n), ints(seed + 2, m, 64), ints(seed + 3, n)
    return Mh, vh, th, yh, ctx.matrix(n, m, Mh), ctx.vector(n, vh)


@pytest.mark.parametrize("m", GEMV_M)
def test_gemv_pair_is_exact_on_integer_data(dev_ctx, m):
    """gemv_t and gemv_n with integer alpha / beta: == per entry; with ncols < m the tail of t (gemv_t: output, gemv_n: input) is
    poisoned -- it must come back bit for bit, and must not be read.  97 .. 132 columns take the one-pass form of lfpsqp_gemv_n."""
    ctx = dev_ctx
    for n in GEMV_N:
        Mh, vh, th, yh, M, v = _gemv_case(ctx, n, m, 100 * m + n)
        for ncols in sorted({m, max(m - 2, 0), (m + 1) // 2}):
            out = ctx.vector(m, np.full(m, POISON))
            L.gemv_t(M, v, out, ncols=ncols)
            got = out.download()
            assert got[:ncols].tolist() == [fsum(Mh[:, j] * vh) for j in range(ncols)]
            assert np.array_equal(bits(got[ncols:]), bits(np.full(m - ncols, POISON)))
            tt = th.copy()
            tt[ncols:] = np.nan                                          # never read
            t = ctx.vector(m, tt)
            acc = np.array([fsum(Mh[i, :ncols] * th[:ncols]) for i in range(n)])
            for alpha, beta in ((2.0, -3.0), (1.0, 0.0), (-1.0, 1.0)):
                y = ctx.vector(n, yh)
                L.gemv_n(M, t, y, alpha, beta, ncols=ncols)
                assert np.array_equal(y.download(), alpha * acc + beta * yh)     # (integers: exact)
                y.free()
            out.free(); t.free()
        assert np.array_equal(M.download(), Mh)
        M.free(); v.free()


@pytest.mark.parametrize("m", [5, 128, 133])
def test_gemv_single_large_entry(dev_ctx, m):
    """gemv_t: v = 2^20 e_p against a matrix of ones (every column sees row p once) and against integer data; gemv_n: t = 2^20 e_p
    picks column p when p < ncols and nothing when p >= ncols."""
    ctx = dev_ctx
    for n in (513, 2049, 4100):
        ones = ctx.matrix(n, m, np.ones((n, m), order="F"))
        Mh = np.asfortranarray(ints(7 * m + n, (n, m)))
        M = ctx.matrix(n, m, Mh)
        out, y, v, t = ctx.vector(m), ctx.vector(n), ctx.vector(n), ctx.vector(m)
        for p in positions_of(n, n):
            v.upload(np.array([BIG]), p)
            L.gemv_t(ones, v, out)
            assert np.all(out.download() == BIG)
            L.gemv_t(M, v, out)
            assert np.array_equal(out.download(), BIG * Mh[p, :])
            v.upload(np.array([0.0]), p)
        ncols = m - 2
        for p in (0, 1, ncols - 1, ncols, m - 1):
            t.upload(np.array([BIG]), p)
            L.gemv_n(M, t, y, 1.0, 0.0, ncols=ncols)
            assert np.array_equal(y.download(), BIG * Mh[:, p] if p < ncols else np.zeros(n))
            t.upload(np.array([0.0]), p)
        for o in (ones, M, out, y, v, t):
            o.free()


# ================================================================================================================================
# (b) the long-vector paths
# ================================================================================================================================
# k * 512 + r rows = k + 1 tiles: more than 3072 partial rows (the four-way unrolled loop of the second stage with its 1024 row
# groups), more than 4096 tiles (two tiles per block), more than 2 * 4096 (three per block, the last block short)
LONG = [(3073 * TILE + 1, 1), (4097 * TILE + 3, 2), (8193 * TILE + 1, 3)]


@pytest.mark.parametrize("n,tiles_per_block", LONG)
def test_long_vectors_are_exact_on_integer_data(dev_ctx, n, tiles_per_block):
    ctx = dev_ctx
    tiles = (n + TILE - 1) // TILE
    tpb = (tiles + 4095) // 4096                                         # vec_grid: at most 4096 blocks for a reduction
    grid = (tiles + tpb - 1) // tpb
    assert tpb == tiles_per_block and grid > (3072 if tpb == 1 else 1) and (tpb < 3 or tiles % tpb != 0)
    xh, yh, th = ints(n, n), ints(n + 1, n), ints(n + 2, n, 8)
    edge = (grid // 2) * tpb * TILE                                      # first row of a block in the middle of the grid
    marks = [0, edge - 1, edge, n - 1]
    for k, p in enumerate(marks):
        xh[p], yh[p], th[p] = (BIG if k % 2 else -BIG), 3.0, 31.0
    x, y, tv = ctx.vector(n, xh), ctx.vector(n, yh), ctx.vector(n, th)
    assert L.dot(x, y) == fsum(xh * yh)
    assert sumsq_shift(x, n, 2.0) == fsum((xh - 2.0) ** 2)
    assert sumsq_shift(x, n - 1, 2.0) == fsum((xh[:-1] - 2.0) ** 2)
    assert separable(1, 0, 3.0, 0.0, tv, n) == fsum(3.0 * th ** 4 + th * th)
    for p in marks:                                                      # the maximum, alone, at each marked place in turn
        x.upload(np.array([2.0 * BIG]), p)
        assert L.amax(x) == 2.0 * BIG
        x.upload(np.array([xh[p]]), p)
    assert L.amax(x) == BIG
    z = ctx.vector(n, np.full(n, POISON))
    L.waxpby(3.0, x, -2.0, y, z)
    assert np.array_equal(z.download(), 3.0 * xh - 2.0 * yh)             # (integers: exact whatever the roundings)
    for v in (x, y, tv, z):
        v.free()


@pytest.mark.parametrize("blocks", [1, 3, 7])
def test_capped_grid_gives_the_same_exact_values(dev_ctx, monkeypatch, blocks):
    """LFPSQP_VEC_BLOCKS caps the grid of vec_kernel, so a block walks several tiles (and the last block fewer) at any length."""
    monkeypatch.setenv("LFPSQP_VEC_BLOCKS", str(blocks))
    ctx = L.Context(0, dev_ctx.L)
    try:
        for n in SIZES:
            _check_integer_reductions(ctx, n, seed=10 * blocks)
            xh, yh = ints(n + blocks, n), ints(n + blocks + 1, n)
            xh[-1], yh[-1] = BIG, -3.0                                   # the last row of the last tile
            x, y, z = ctx.vector(n, xh), ctx.vector(n, yh), ctx.vector(n, np.full(n, POISON))
            assert L.dot(x, y) == fsum(xh * yh) and L.amax(x) == BIG
            L.waxpby(3.0, x, -2.0, y, z)
            assert np.array_equal(z.download(), 3.0 * xh - 2.0 * yh)
            for v in (x, y, z):
                v.free()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gemv_t_two_stage_reduction_is_exact(gpu_lib):
    """m = 32 columns over 2048 * 2048 + 3 rows (about 1.1 GB): launch_reduce takes its two-stage form for >= 32 columns and
    >= 2048 partial rows, which no other direct test of the product reaches."""
    ctx = L.Context(0, gpu_lib)
    try:
        n, m = 2048 * 2048 + 3, 32
        ks = 4 if n >= 4000000 else 2                                    # lfpsqp_ctx::ks_for with the default tuning
        partial_rows = (n + TILE * ks - 1) // (TILE * ks)                # ntiles_of(n, ks)
        assert partial_rows >= 2048 and m >= 32
        rng = np.random.default_rng(5)
        Mh = np.empty((n, m), order="F")
        for j in range(m):
            Mh[:, j] = rng.integers(-1024, 1025, n)
        vh = ints(6, n)
        vh[0], vh[-1], vh[2048 * 1024] = BIG, -BIG, BIG
        M, v, out = ctx.matrix(n, m, Mh), ctx.vector(n, vh), ctx.vector(m)
        L.gemv_t(M, v, out)
        got = out.download()
        for j in range(m):
            assert got[j] == fsum(Mh[:, j] * vh), j
    finally:
        ctx.close()


# ================================================================================================================================
# (c) rounding-error bounds on hostile real data
# ================================================================================================================================
def _cancelling_pair(seed, n):
    """x, y of <= 26 significant bits, entries over 2^-30 .. 2^30, the second half mirroring the first with y negated (shuffled): the
    exact sum of products is the unpaired tiny term of an odd n (zero for an even n), far below 1e-10 * sum |x_i y_i|."""
    h = n // 2
    xa, ya = short_reals(seed, h), short_reals(seed + 1, h)
    xh, yh = np.concatenate([xa, xa, [2.0 ** -30] * (n - 2 * h)]), np.concatenate([ya, -ya, [2.0 ** -30] * (n - 2 * h)])
    perm = np.random.default_rng(seed + 2).permutation(n)
    return xh[perm], yh[perm]


@pytest.mark.parametrize("n", [65, 513, 2048, 2049, 4097])
def test_dot_error_bound_on_cancelling_data(dev_ctx, n):
    """DotF: a term x_i y_i is rounded once (or not at all where it is fused into an addition) and then passes through at most
    n - 1 additions, in whatever order the lanes, waves, blocks and the second stage take them: k = n roundings, + 1 spare for the
    additions of a zero-initialised accumulator = n + 1, and |computed - exact| <= gamma_{n+1} sum |x_i y_i|."""
    ctx = dev_ctx
    xh, yh = _cancelling_pair(n, n)
    terms = [Fraction(a) * Fraction(b) for a, b in zip(xh.tolist(), yh.tolist())]
    exact, mag = sum(terms), sum(abs(t) for t in terms)
    assert abs(exact) <= Fraction(1e-10) * mag                           # the data is as hostile as intended
    x, y = ctx.vector(n, xh), ctx.vector(n, yh)
    got = L.dot(x, y)
    print(f"dot n={n}: |err| = {float(abs(Fraction(got) - exact)):.3e}, bound = {float(gamma(n + 1) * mag):.3e}")
    assert abs(Fraction(got) - exact) <= gamma(n + 1) * mag
    c = n - 1
    ex_c, mag_c = sum(terms[:c]), sum(abs(t) for t in terms[:c])
    assert abs(Fraction(dot_head(x, y, c)) - ex_c) <= gamma(n + 1) * mag_c


@pytest.mark.parametrize("n", [3, 513, 2049, 4097])
def test_sumsq_shift_error_bound_near_the_shift(dev_ctx, n):
    """SumSqShiftF: d = fl(x - c) enters the product twice (2), the product is rounded once or fused (1), then at most n - 1
    additions: k = n + 2, + 1 spare = n + 3, and the bound is gamma_{n+3} * sum (x_i - c)^2 (all terms positive).  x lies from 2^-30
    to 2^30 away from c = 1/3, so x - c is a rounded (often cancelling) difference for most entries."""
    ctx = dev_ctx
    c = 1.0 / 3.0
    xh = c + reals(n + 40, n)
    terms = [(Fraction(a) - Fraction(c)) ** 2 for a in xh.tolist()]
    x = ctx.vector(n, xh)
    for count in (n, n - 1):
        exact = sum(terms[:count])
        got = sumsq_shift(x, count, c)
        print(f"sumsq_shift n={n} count={count}: rel err = {float(abs(Fraction(got) - exact) / exact):.3e}, gamma = {float(gamma(n + 3)):.3e}")
        assert abs(Fraction(got) - exact) <= gamma(n + 3) * exact


@pytest.mark.parametrize("n,m", [(513, 5), (2049, 37), (1025, 130)])
def test_gemv_t_error_bound_on_cancelling_data(dev_ctx, n, m):
    """gemv_t, per column j: n products (fused into the running sums) and at most n - 1 additions over lanes, waves, tiles and the
    second stage: |computed - exact|_j <= gamma_{n+1} (|M|' |v|)_j.  The lower half of the rows mirrors the upper half with v
    negated, so every exact column sum is the single unpaired term."""
    ctx = dev_ctx
    h = n // 2
    top = np.stack([short_reals(1000 * j + n, h) for j in range(m)], axis=1)
    last = np.ldexp(np.ones((n - 2 * h, m)), -30)
    va = short_reals(n + m, h)
    vh = np.concatenate([va, -va, [2.0 ** -30] * (n - 2 * h)])
    perm = np.random.default_rng(n).permutation(n)
    Mh, vh = np.asfortranarray(np.concatenate([top, top, last])[perm]), vh[perm]
    M, v, out = ctx.matrix(n, m, Mh), ctx.vector(n, vh), ctx.vector(m)
    L.gemv_t(M, v, out)
    got = out.download()
    vf = [Fraction(a) for a in vh.tolist()]
    for j in range(m):
        terms = [Fraction(a) * b for a, b in zip(Mh[:, j].tolist(), vf)]
        exact, mag = sum(terms), sum(abs(t) for t in terms)
        assert abs(exact) <= Fraction(1e-10) * mag
        assert abs(Fraction(got[j]) - exact) <= gamma(n + 1) * mag, j


@pytest.mark.parametrize("n,m", [(513, 5), (1025, 37), (1025, 129), (2049, 133)])
def test_gemv_n_error_bound_on_cancelling_data(dev_ctx, n, m):
    """gemv_n, per row i: acc = sum_j M_ij t_j (m fused products, at most m - 1 additions), then fl(alpha acc + fl(beta y_i)): a term
    of the sum meets at most m roundings and the one of the final fused operation, beta y_i two: |computed - exact|_i <=
    gamma_{m+2} (|alpha| |M| |t| + |beta y|)_i.  The right half of the columns mirrors the left half with t negated (entries over
    2^-10 .. 2^10, the unpaired column 2^-30 * 2^-30); m = 129 runs on the one-pass form, the others on the two-pass kernels."""
    ctx = dev_ctx
    h = m // 2
    left = np.stack([short_reals(77 * j + n, n, -10, 10) for j in range(h)], axis=1)
    ta = short_reals(n + m, h, -10, 10)
    th = np.concatenate([ta, -ta, [2.0 ** -30] * (m - 2 * h)])
    perm = np.random.default_rng(m).permutation(m)
    Mh = np.asfortranarray(np.concatenate([left, left, np.ldexp(np.ones((n, m - 2 * h)), -30)], axis=1)[:, perm])
    th = th[perm]
    yh = reals(n + 5, n, -25, -15)
    alpha, beta = 0.7, -1.3
    M, t, y = ctx.matrix(n, m, Mh), ctx.vector(m, th), ctx.vector(n, yh)
    L.gemv_n(M, t, y, alpha, beta)
    got = y.download()
    tf = [Fraction(a) for a in th.tolist()]
    fa, fb = Fraction(alpha), Fraction(beta)
    for i in range(n):
        terms = [Fraction(a) * b for a, b in zip(Mh[i, :].tolist(), tf)]
        s, sa = sum(terms), sum(abs(q) for q in terms)
        assert abs(s) <= Fraction(1e-10) * sa
        exact, mag = fa * s + fb * Fraction(yh[i]), abs(fa) * sa + abs(fb * Fraction(yh[i]))
        assert abs(Fraction(got[i]) - exact) <= gamma(m + 2) * mag, i


# ================================================================================================================================
# (d) elementwise maps, entry by entry
# ================================================================================================================================
def waxpby_ref(a, xh, b, yh):
    """WaxpbyF: a*x when b == 0 (y not read), else b*y when a == 0 (x not read), else fma(a, x, fl(b*y)) -- the explicit fma is one
    value on the emulator and on the GPU; so is every single product (nothing to contract)."""
    fa, fb = Fraction(a), Fraction(b)
    if b == 0.0:
        return [rnd(fa * Fraction(p)) for p in xh.tolist()]
    if a == 0.0:
        return [rnd(fb * Fraction(q)) for q in yh.tolist()]
    return [rnd(fa * Fraction(p) + Fraction(rnd(fb * Fraction(q)))) for p, q in zip(xh.tolist(), yh.tolist())]


@pytest.mark.parametrize("n", [1, 2, 513, 2047, 2049, 4097])
def test_waxpby_axpby_vmul_entry_by_entry_with_aliasing(dev_ctx, n):
    """Each output entry == the functor's expression with one rounding per machine operation; z may be x, y, or both."""
    ctx = dev_ctx
    xh, yh = reals(n, n), reals(n + 1, n)
    a, b = 0.3, -1.7
    x, y, z = ctx.vector(n, xh), ctx.vector(n, yh), ctx.vector(n, np.full(n, POISON))
    L.waxpby(a, x, b, y, z)
    assert z.download().tolist() == waxpby_ref(a, xh, b, yh)
    assert np.array_equal(x.download(), xh) and np.array_equal(y.download(), yh)
    L.waxpby(a, x, b, y, x)                                              # z is x
    assert x.download().tolist() == waxpby_ref(a, xh, b, yh)
    x.upload(xh)
    L.waxpby(a, x, b, y, y)                                              # z is y
    assert y.download().tolist() == waxpby_ref(a, xh, b, yh)
    L.waxpby(a, x, b, x, x)                                              # x is y is z
    assert x.download().tolist() == waxpby_ref(a, xh, b, xh)
    x.upload(xh); y.upload(yh)
    L.axpby(a, x, b, y)
    assert y.download().tolist() == waxpby_ref(a, xh, b, yh)
    y.upload(yh)
    prod = [rnd(Fraction(p) * Fraction(q)) for p, q in zip(xh.tolist(), yh.tolist())]
    L.vmul(x, y, z)
    assert z.download().tolist() == prod
    L.vmul(x, y, y)                                                      # the output is the second factor
    assert y.download().tolist() == prod
    y.upload(yh)
    L.vmul(x, y, x)                                                      # the output is the diagonal
    assert x.download().tolist() == prod
    x.upload(xh)
    L.vmul(x, x, x)
    assert x.download().tolist() == [rnd(Fraction(p) ** 2) for p in xh.tolist()]


@pytest.mark.parametrize("n", [1, 2, 513, 2049])
def test_zero_coefficients_never_read_the_other_operand(dev_ctx, n):
    """b == 0 with NaN and Inf planted in y, a == 0 with NaN in x: finite outputs equal to the reference (BLAS semantics)."""
    ctx = dev_ctx
    xh, yh = reals(n + 2, n), reals(n + 3, n)
    bad = yh.copy()
    bad[::2], bad[1::2], bad[-1] = np.nan, np.inf, -np.inf
    x, y, z = ctx.vector(n, xh), ctx.vector(n, bad), ctx.vector(n, np.full(n, np.nan))
    L.waxpby(1.5, x, 0.0, y, z)
    assert z.download().tolist() == waxpby_ref(1.5, xh, 0.0, bad)
    L.waxpby(0.0, y, -0.5, x, z)                                         # a == 0: the NaNs sit in the first operand now
    assert z.download().tolist() == waxpby_ref(0.0, bad, -0.5, xh)
    L.axpby(1.5, x, 0.0, y)                                              # y = 1.5 x + 0 y over a y full of NaN
    assert y.download().tolist() == waxpby_ref(1.5, xh, 0.0, bad)


@pytest.mark.parametrize("m", [5, 96, 128, 132])
def test_gemv_n_beta_zero_never_reads_y(dev_ctx, m):
    """AxpbyEpi (two-pass, m = 5 and 96) and GemvNRow (one-pass, m = 128 and 132): beta == 0 over a y full of NaN and Inf."""
    ctx = dev_ctx
    for n in (513, 2049, 4100):
        Mh, vh, th, yh, M, v = _gemv_case(ctx, n, m, 3 * m + n)
        bad = np.full(n, np.nan)
        bad[1::3] = np.inf
        y, t = ctx.vector(n, bad), ctx.vector(m, th)
        L.gemv_n(M, t, y, -2.0, 0.0)
        got = y.download()
        assert np.all(np.isfinite(got))
        assert got.tolist() == [-2.0 * fsum(Mh[i, :] * th) for i in range(n)]
        for o in (M, v, y, t):
            o.free()


HEADS = [(2048, 1023), (2049, 1024), (512, 511), (513, 512), (514, 513), (1026, 513), (4097, 2048), (4096, 2049), (2, 1), (3, 2), (1, 1)]


@pytest.mark.parametrize("n,count", HEADS)
def test_affine_head_and_separable_leave_the_tail_untouched(dev_ctx, n, count):
    """y[i] = fma(a, x[i], c) for i < count, exactly; every entry >= count keeps its bits -- odd count inside an even length (the
    pair store must fall back to a scalar store), even count inside an odd length, counts on a tile edge and one either side."""
    ctx = dev_ctx
    xh = reals(n + count, n)
    a, c = 2.0 / 3.0, -0.1
    x, y = ctx.vector(n, xh), ctx.vector(n, np.full(n, POISON))
    affine_head(a, x, c, count, y)
    got = y.download()
    assert got[:count].tolist() == [fma(a, p, c) for p in xh[:count].tolist()]
    assert np.array_equal(bits(got[count:]), bits(np.full(n - count, POISON)))
    affine_head(a, x, c, 0, y)                                           # count == 0: nothing at all
    assert np.array_equal(bits(y.download()), bits(got))
    th = ints(n, n, 8)
    tv = ctx.vector(n, th)
    for kind in (0, 1, 2):
        for mode in (1, 2):
            y.fill(POISON)
            separable(kind, mode, 2.0, 0.0, tv, count, y)
            got = y.download()
            assert np.array_equal(bits(got[count:]), bits(np.full(n - count, POISON))), (kind, mode)
            assert not np.any(got[:count] == POISON)
            if kind < 2:                                                 # (integers: exact)
                ref = {(0, 1): 4.0 * th, (0, 2): np.full(n, 4.0), (1, 1): 8.0 * th ** 3 + 2.0 * th, (1, 2): 24.0 * th * th + 2.0}[(kind, mode)]
                assert np.array_equal(got[:count], ref[:count])


RANGES = [(1, 5), (3, 509), (3, 510), (511, 1), (511, 2), (512, 1), (512, 512), (513, 511), (509, 1027), (1, 2047), (0, 513), (1023, 1026),
          (2047, 2), (2049, 1), (2050, 0)]


@pytest.mark.parametrize("n", [2050, 2051])
def test_fill_range_and_copy_range_touch_their_range_only(dev_ctx, n):
    """Ranges that start and end inside a tile, on a tile edge and one past it, odd offsets included: the addressed entries get
    the value, every other entry keeps its bits."""
    ctx = dev_ctx
    src_h = reals(n, n)
    src = ctx.vector(n, src_h)
    v = ctx.vector(n)
    for off, cnt in RANGES:
        v.fill(POISON)
        fill_range(v, off, cnt, 2.5)
        ref = np.full(n, POISON)
        ref[off:off + cnt] = 2.5
        assert np.array_equal(bits(v.download()), bits(ref)), (off, cnt)
        for src_off in (0, 1, n - off - cnt):
            v.fill(POISON)
            v.copy_range_from(src, cnt, off, src_off)
            ref = np.full(n, POISON)
            ref[off:off + cnt] = src_h[src_off:src_off + cnt]
            assert np.array_equal(bits(v.download()), bits(ref)), (off, cnt, src_off)
    assert np.array_equal(src.download(), src_h)


@pytest.mark.parametrize("N", [700, 2049])
def test_stacked_vectors_keep_their_gap_zero(dev_ctx, N):
    """include/lfpsqp_hip.h: x-half at [0, N), y-half at [hs, hs + N), "gap kept zero, every BLAS-1 primitive works on it
    unchanged".  After waxpby / axpby / vmul / copy_from between stacked vectors the gap is zero and dot / nrm2 / amax over the
    stacked length are the exact values over the 2N logical entries; fill and hash_fill write the two halves only."""
    ctx = dev_ctx
    ah, bh = ints(N, 2 * N), ints(N + 1, 2 * N)
    a, b, z = StackedVector(ctx, N).upload2(ah), StackedVector(ctx, N).upload2(bh), StackedVector(ctx, N)
    hs = a.hs
    assert hs > N and hs % 2048 == 0 and a.n == hs + N

    def gap(v):
        return v.download(hs - N, N)

    assert L.dot(a, b) == fsum(ah * bh) and L.nrm2(a) == math.sqrt(fsum(ah * ah)) and L.amax(a) == np.abs(ah).max()
    L.waxpby(3.0, a, -2.0, b, z)
    assert np.array_equal(z.download2(), 3.0 * ah - 2.0 * bh) and not gap(z).any()
    assert L.dot(z, b) == fsum((3.0 * ah - 2.0 * bh) * bh) and L.amax(z) == np.abs(3.0 * ah - 2.0 * bh).max()
    L.axpby(2.0, a, 5.0, z)
    assert np.array_equal(z.download2(), 2.0 * ah + 5.0 * (3.0 * ah - 2.0 * bh)) and not gap(z).any()
    L.vmul(a, b, z)
    assert np.array_equal(z.download2(), ah * bh) and not gap(z).any()
    assert L.nrm2(z) == math.sqrt(fsum((ah * bh) ** 2))
    z.copy_from(a)
    assert np.array_equal(z.download2(), ah) and not gap(z).any()
    z.fill(3.0)
    assert np.all(z.download2() == 3.0) and not gap(z).any()
    assert L.dot(z, z) == 9.0 * 2 * N and L.amax(z) == 3.0
    z.fill(0.0)
    assert not z.download().any()
    z.hash_fill(9, 5, 4.0, 5.0)                                          # logical entry k = scale * u(seed, offset + k) + shift
    plain = ctx.vector(2 * N).hash_fill(9, 5, 4.0, 5.0).download()
    assert np.array_equal(z.download2(), plain) and not gap(z).any()
    assert L.amax(z) == np.abs(plain).max()


# ================================================================================================================================
# (e) lfpsqp_separable against a 60-digit statement of its definition
# ================================================================================================================================
def sep_true(kind, mode, a, x, c):
    """The definition in include/lfpsqp_hip.h -- kind 0: a t^2, 1: a t^4 + t^2, 2: a (sqrt(1 + t^2) - 1); mode 0 / 1 / 2: phi, phi',
    phi'' -- in the decimal arithmetic of the caller's context (60 digits) from the EXACT difference t = x - c (a Fraction, rounded
    to 60 digits once).  |t| >= 2^-31 on the grid, so sqrt(1 + t^2) - 1 >= 1e-19 keeps 40 correct digits."""
    t = Fraction(x) - Fraction(c)
    t = decimal.Decimal(t.numerator) / decimal.Decimal(t.denominator)
    a = decimal.Decimal(a)
    if kind == 0:
        return [a * t * t, 2 * a * t, 2 * a][mode]
    if kind == 1:
        return [a * t ** 4 + t * t, 4 * a * t ** 3 + 2 * t, 12 * a * t * t + 2][mode]
    s = (1 + t * t).sqrt()
    return [a * (s - 1), a * t / s, a / (s * s * s)][mode]


# relative error of sep_eval in units of u, derived in the docstring of test_separable_to_a_relative_bound
SEP_K = {(0, 0): 4, (0, 1): 2, (0, 2): 0, (1, 0): 8, (1, 1): 6, (1, 2): 5, (2, 0): 8, (2, 1): 6, (2, 2): 11}


def _sep_grid(seed):
    """t over {0} u {+-2^-k, k = 1..30} u {+-2^k, k = 0..30} and hashed values in between; c of a few bits so that x = c + t is exact
    for the powers of two, and a full-mantissa x elsewhere (t is then whatever x - c is: the reference uses the exact difference)."""
    rng = np.random.default_rng(seed)
    pw = [0.0] + [s * 2.0 ** -k for k in range(1, 31) for s in (1, -1)] + [s * 2.0 ** k for k in range(0, 31) for s in (1, -1)]
    t = np.concatenate([pw, reals(seed + 1, 200)])
    c = rng.integers(-4, 5, t.size) * 0.25
    a = rng.uniform(0.5, 1.5, t.size)
    return a, c, c + t


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_separable_to_a_relative_bound(dev_ctx, kind, mode):
    """Every value of phi, phi', phi'' to a RELATIVE error of gamma_k ~ k u.  k counts, to first order, the roundings of sep_eval
    (csrc/primitives.hip) on the way to the value, each weighted by how it enters, plus the rounding of t = fl(x - c) times the power
    of t in the term; a > 0, so the two terms of kind 1 have one sign and the larger count holds for their sum.
      kind 0   a*t*t: 2 products + t twice = 4;   2.0*a*t: 2a is exact, 1 product + t = 2;   2.0*a: exact, 0.
      kind 1   t2 = fl(t*t) carries 2 + 1 = 3.  mode 0, fma(a*t2, t2, t2): the quartic term 3 + 3 (t2 twice) + 1 (a*t2) + 1 (fma) = 8.
               mode 1, fma(4.0*a*t2, t, 2.0*t): 4a exact, 3 (t2) + 1 (product) + 1 (t) + 1 (fma) = 6.   mode 2, fma(12.0*a, t2, 2.0):
               1 (12a) + 3 (t2) + 1 (fma) = 5.
      kind 2   w = fma(t, t, 1): one rounding, and the error of t enters 1 + t^2 with the weight 2 theta, theta = t^2 / (1 + t^2) < 1;
               s = sqrt(w) halves both and adds its own: s carries at most 1/2 + theta + 1 <= 2.5.
               mode 0, a*t*t/(s + 1.0): 2 products, the addition, the division = 4; t twice = 2; s with the weight s / (s + 1) < 1,
               of which the theta part partly cancels against t's own: at most 1.5 more -- 7.5, taken as 8.
               mode 1, a*t/s: product, division, t = 3, and s: 2.5 -- 5.5, taken as 6.
               mode 2, a/(s*s*s): 2 products and the division = 3, and s three times: 7.5 -- 10.5, taken as 11.
    Mode 0 is also checked as a sum over the grid against gamma_{n + k} * sum phi (positive terms).  The relative bound is the
    point: kind 2 mode 0 evaluated as a*(s - 1.0) has a relative error of up to 2^-53 / t^2 and returns 0 for |t| <= 2^-27 (measured
    with that expression on the emulator: 1.1e-13 at t = 2^-10 and 2.3e-13 at 2^-20 -- powers of two are kind to it, 1 + t^2 being
    exact there --, 1.0 at 2^-27; 284 of the 646 values of the grid miss the bound, from |t| = 0.125 down)."""
    ctx = dev_ctx
    ah, ch, xh = _sep_grid(100 * kind + mode)
    n = xh.size
    k = SEP_K[(kind, mode)]
    x, av, cv, out = ctx.vector(n, xh), ctx.vector(n, ah), ctx.vector(n, ch), ctx.vector(n)
    x1, a1, c1 = ctx.vector(1), ctx.vector(1), ctx.vector(1)
    worst, bad = 0.0, []
    with decimal.localcontext() as dc:
        dc.prec = 60
        tol = decimal.Decimal(gamma(k).numerator) / decimal.Decimal(gamma(k).denominator)
        tol_sum = decimal.Decimal(gamma(n + k).numerator) / decimal.Decimal(gamma(n + k).denominator)
        for per_variable in (True, False):
            aa = ah if per_variable else np.full(n, 1.25)
            cc = ch if per_variable else np.full(n, 0.25)
            xx = xh if per_variable else cc + (xh - ch)
            x.upload(xx)
            A, Cc = (av, cv) if per_variable else (1.25, 0.25)
            true = [sep_true(kind, mode, p, q, r) for p, q, r in zip(aa.tolist(), xx.tolist(), cc.tolist())]
            if mode == 0:
                got = []
                for i in range(n):                                       # elementwise: count = 1 calls on one-entry vectors
                    x1.upload(xx[i:i + 1]); a1.upload(aa[i:i + 1]); c1.upload(cc[i:i + 1])
                    got.append(separable(kind, 0, a1 if per_variable else 1.25, c1 if per_variable else 0.25, x1, 1))
                total, ex = separable(kind, 0, A, Cc, x, n), sum(true)
                assert abs(decimal.Decimal(total) - ex) <= tol_sum * ex
            else:
                separable(kind, mode, A, Cc, x, n, out)
                got = out.download().tolist()
            for i in range(n):
                t = xx[i] - cc[i]
                if true[i] == 0:
                    assert got[i] == 0.0, (i, xx[i], cc[i])
                    continue
                rel = abs((decimal.Decimal(got[i]) - true[i]) / true[i])
                worst = max(worst, float(rel))
                if kind == 2 and mode == 0 and per_variable and t in (2.0 ** -10, 2.0 ** -20, 2.0 ** -27):
                    print(f"kind 2 mode 0, t = 2^{int(math.log2(t))}: relative error {float(rel):.3e}")
                if not rel <= tol:
                    bad.append((per_variable, i, xx[i], cc[i], got[i], float(true[i]), f"{float(rel) / U:.3g} u"))
    print(f"separable kind {kind} mode {mode}: worst relative error {worst / U:.2f} u, bound {k} u")
    assert not bad, (len(bad), bad[:5])                                  # (every figure is printed before the one assertion on them)
