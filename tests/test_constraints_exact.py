"""The constraint family (lfpsqp_constraints_eval / _jac / _hess_diag: csrc/retract.hip -- cons_raw, cons_eval, BallF, BallColF, EwEvalE,
EwDerivF, ew_jac_kernel, EwHessE, EwHessVecF, NRStepE in its eval_only form through onepass_kernel) and the sparse products underneath
(lfpsqp_spmv_t / _n, lfpsqp_spmat_rowscale, lfpsqp_spmat_to_dense: csrc/sparse.hip) against exactly rounded references.

Every reference is computed on the host with int64 numpy products of integer data, `fractions.Fraction`, `math.fsum` over products that
are exact by construction, or `mpmath` at 80 digits (sin, cos); floating-point numpy sums, BLAS and scipy products are never a reference.

  (a) c!, jac! and the Hessian diagonal on integer data (|A_ij| <= 16, |x_i| <= 8, kinds {t, t^2}, |qw|, |lam|, |b| <= 4): every product
      and partial sum in any order is an integer far below 2^53, so the assertion is == -- over the four storage forms of the nonlinear
      class and the linear class, the row counts either side of a 64-row round and a 512-row tile, every n_x edge, every tile class of
      run_onepass and the run_gemv_nt shapes, the column blocks of ew_jac_kernel, ball and slack, and a single 2^20;
  (b) the sin kind: the device's own sin / cos measured in ulps against mpmath, then entrywise a-priori bounds;
  (c) the sparse products: == on integer data at the column lengths where spmv_t changes path, then cancelling real data;
  (d) (GPU only) row counts at which a workgroup of the c! launch takes several rounds.

x, hx and kind are allocated PAD entries longer than n with NaN, POISON and kind 1 (sin) in the tail: nothing beyond row n may reach a
result or be written.  Each case runs on the CPU emulator build and, under -m gpu, on the MI355X, with the same assertions."""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import lfpsqp_jl_amd as L
from tests.helpers import POISON, U, bits, fsum, gamma, i64, imatmul, ints, short_reals, ulp

BIG = 2.0 ** 20                                  # the sentinel
PAD = 3                                          # (odd: for even n the first tail entry shares a 16-byte piece with nothing, for odd n with row n - 1)
LIM_A, LIM_X, LIM_S = 16, 8, 4                   # |A_ij|, |x_i|, |qw_j| / |lam_j| / |b_j|
R2 = 37
ROWS = [1, 2, 3, 63, 64, 65, 127, 129, 511, 513, 1025, 2049]
mpmath.mp.prec = 280                             # (> 80 digits)


def padded(ctx, a, fill):
    """a on the device in a vector PAD entries longer, the tail holding `fill`."""
    return ctx.vector(len(a) + PAD, np.concatenate([np.asarray(a, dtype=np.float64), np.full(PAD, fill)]))


def sparse_pattern(seed, n, m, kmax=5):
    """0 .. kmax entries per row (about one row in eight empty; at least one row has none when n > 8), column m // 2 empty when m > 2:
    (rows, cols), unsorted."""
    rng = np.random.default_rng(seed)
    allowed = np.array([j for j in range(m) if not (m > 2 and j == m // 2)])
    rows, cols = [], []
    for i in range(n):
        k = 0 if (rng.random() < 0.125 or (n > 8 and i == n // 3)) else int(rng.integers(1, min(kmax, len(allowed)) + 1))
        for j in rng.choice(allowed, k, replace=False):
            rows.append(i)
            cols.append(int(j))
    p = rng.permutation(len(rows))
    return np.array(rows, dtype=np.int64)[p], np.array(cols, dtype=np.int64)[p]


def nonzero_ints(seed, k, lim):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, lim + 1, k) * rng.choice([-1, 1], k)).astype(np.float64)


class System:
    """One constraint object with its integer data on the host (int64: Ai, xi, ki, qi, bi, h0i; lam) and on the device.

    form: "dense" (ElementwiseConstraints, materialised gradients), "stream" (a view of A), "sparse" (A a SparseMatrix),
    "linear" / "linear-sp" (DeviceConstraints without / with Jsp).  A caller-owned Jct has two columns more than the class uses, POISON."""

    def __init__(self, ctx, form, n, m, seed, qw=False, ball=False, kinds=(0, 2), Ah=None, xh=None, kh=None):
        self.ctx, self.form, self.n, self.m, self.ball = ctx, form, n, m, ball
        self.linear = form.startswith("linear")
        self.sparse = form in ("sparse", "linear-sp")
        rng = np.random.default_rng(seed)
        if Ah is None:
            if self.sparse:
                r, c = sparse_pattern(seed + 11, n, m)
                Ah = np.zeros((n, m))
                Ah[r, c] = nonzero_ints(seed + 12, len(r), LIM_A)
            else:
                Ah = ints(seed, (n, m), LIM_A)
        self.Ah = np.asfortranarray(Ah, dtype=np.float64)
        if self.sparse:
            r, c = np.nonzero(self.Ah)
            p = rng.permutation(len(r))                                    # (triplets in no particular order)
            self.Asp = L.SparseMatrix(ctx, n, m, r[p], c[p], self.Ah[r[p], c[p]])
        self.xh = ints(seed + 1, n, LIM_X) if xh is None else np.asarray(xh, dtype=np.float64)
        if kh is None:
            kh = np.zeros(n) if self.linear else rng.choice(np.asarray(kinds, dtype=np.float64), n)
        self.kh = kh
        self.qh = nonzero_ints(seed + 2, m, LIM_S) if qw else None
        self.bh = ints(seed + 3, m, LIM_S)
        self.lam = ints(seed + 4, m + 1, LIM_S)
        self.lam[-1] = 3.0
        self.h0 = ints(seed + 5, n, 1024)
        self.x = padded(ctx, self.xh, np.nan)
        self.kind = None if self.linear else padded(ctx, self.kh, 1.0)
        self.hx = padded(ctx, self.h0, POISON)
        mt = m + (1 if ball else 0)
        self.mt = mt
        if form == "stream":
            self.A = ctx.matrix(n, m, self.Ah)
            self.cons = L.ElementwiseConstraints(ctx, self.A, self.bh, kind=self.kind, qw=self.qh, stream=True)
        else:
            self.Jct = ctx.matrix(n, mt + 2)
            self.Jct.upload(np.full((n, mt + 2), POISON))
            if form == "dense":
                self.A = ctx.matrix(n, m, self.Ah)
                self.cons = L.ElementwiseConstraints(ctx, self.A, self.bh, kind=self.kind, qw=self.qh, Jct=self.Jct, has_ball=ball, R2=R2, stream=False)
            elif form == "sparse":
                assert not qw
                self.cons = L.ElementwiseConstraints(ctx, self.Asp, self.bh, kind=self.kind, Jct=self.Jct, has_ball=ball, R2=R2)
            else:
                assert not qw
                if m:
                    self.Jct.upload(self.Ah)
                self.cons = L.DeviceConstraints(self.Jct, m, self.bh, has_ball=ball, R2=R2, Jsp=self.Asp if self.sparse else None)
        self.Ai, self.xi, self.ki, self.bi, self.h0i = i64(self.Ah), i64(self.xh), i64(self.kh), i64(self.bh), i64(self.h0)
        self.qi = i64(self.qh) if qw else np.zeros(m, dtype=np.int64)
        self.li = i64(self.lam)

    def check_limits(self):
        """The limits under which every partial sum is an integer below 2^53 (16 * 64 * n at the most)."""
        assert np.abs(self.Ai).max(initial=0) <= LIM_A and np.abs(self.xi).max() <= LIM_X and set(np.unique(self.ki)) <= {0, 2}
        assert max(np.abs(self.qi).max(initial=0), np.abs(self.bi).max(initial=0), np.abs(self.li).max()) <= LIM_S
        assert LIM_A * LIM_X * LIM_X * self.n + 2 * LIM_S * LIM_X * LIM_X * self.n < 2 ** 40

    def reference(self, n_x, slack):
        """int64: (c, Jct[:, :mt], h0 + the Hessian diagonal, rs = phi'(x), u = 2 x [i < n_x])."""
        x, A, k, n, m = self.xi, self.Ai, self.ki, self.n, self.m
        below = (np.arange(n) < n_x).astype(np.int64)
        phi = np.where(k == 0, x, x * x)
        d1 = np.where(k == 0, 1, 2 * x)
        d2 = np.where(k == 0, 0, 2)
        q = int((x * x * below).sum())
        c = np.zeros(self.mt, dtype=np.int64)
        c[:m] = imatmul(A.T, phi) + self.qi * q - self.bi
        J = np.zeros((n, self.mt), dtype=np.int64)
        J[:, :m] = d1[:, None] * A + np.outer(2 * x * below, self.qi)
        cq = 2 * int(self.qi @ self.li[:m])
        if self.ball:
            c[m] = q - (int(x[slack]) if slack >= 0 else 0) - R2
            J[:, m] = 2 * x * below
            if slack >= 0:
                assert n_x <= slack < n
                J[slack, m] = -1
            cq += 2 * int(self.li[m])
        h = self.h0i + d2 * imatmul(A, self.li[:m]) + cq * below
        for v in (c, J, h):                                                # (exactly representable: the device can hold the reference)
            assert np.array_equal(v.astype(np.float64).astype(np.int64), v)
        return c, J, h, d1, 2 * x * below

    def check(self, n_x, slack=-1, what=("c", "jac", "hess")):
        """c!, jac! and hess_diag at (n_x, slack_row) against the int64 reference, ==; the tails and the spare columns keep their bits."""
        cons, n, m, mt = self.cons, self.n, self.m, self.mt
        cons.n_x, cons.slack_row = n_x, slack
        c, J, h, d1, u2 = self.reference(n_x, slack)
        tag = (self.form, n, m, n_x, slack)
        x0 = bits(self.x.download())
        cv = np.full(mt + 1, POISON)
        if "c" in what:
            cons.c_(cv, self.x)
            assert np.array_equal(cv[:mt], c), tag
            assert cv[mt] == POISON
        if "jac" in what:
            cvj, cvn = np.full(mt + 1, POISON), np.full(mt + 1, POISON)
            cons.jac_(cons.Jct, cvn, self.x, evaluate=False)
            assert np.all(cvn == POISON), tag                              # the gradients only: cval untouched
            cons.jac_(cons.Jct, cvj, self.x)
            if "c" in what:
                assert np.array_equal(bits(cvj), bits(cv)), tag            # jac! evaluates the same c!
            assert np.array_equal(cvj[:mt], c), tag
            Jd = cons.Jct.download()
            bad = np.argwhere(Jd[:, :mt] != J)
            assert bad.size == 0, (tag, bad[:4], Jd[:, :mt][tuple(bad[0])], J[tuple(bad[0])])
            if self.form == "stream":
                if cons.rs is not None:
                    assert np.array_equal(cons.rs.download(), d1), tag
                if cons.ru is not None:
                    assert np.array_equal(cons.ru.download(), u2), tag
            else:
                lo = mt if (self.ball or not self.linear) else m           # (the linear class without a ball writes no column at all)
                assert np.all(Jd[:, lo:] == POISON), tag
                if self.linear and not self.ball and m:
                    assert np.array_equal(Jd[:, :m], self.Ah)
            if self.form == "sparse":
                assert np.array_equal(cons.Jsp.to_dense().download(), J[:, :m]), tag
        if "hess" in what:
            self.hx.upload(np.concatenate([self.h0, np.full(PAD, POISON)]))
            cons.hess_diag_(self.hx, self.x, self.lam[:max(mt, 1)])
            out = self.hx.download()
            bad = np.argwhere(out[:n] != h)
            assert bad.size == 0, (tag, bad[:4].ravel(), out[:n][bad[:4].ravel()], h[bad[:4].ravel()])
            assert np.all(out[n:] == POISON), tag
            if self.linear:                                                # only the ball term: the rows from n_x on keep their bits
                assert np.array_equal(bits(out[n_x:n]), bits(self.h0[n_x:])), tag
        assert np.array_equal(bits(self.x.download()), x0), tag
        if self.kind is not None:
            assert np.array_equal(self.kind.download(), np.concatenate([self.kh, np.ones(PAD)]))


def nx_edges(n):
    """0, 1, n - 1, n, and an odd and an even value in between."""
    mid = n // 2
    return sorted({v for v in (0, 1, n - 1, n, mid | 1, (mid | 1) + 1) if 0 <= v <= n})


def slack_for(n, n_x, turn):
    """-1, n_x, n - 1 in turn, where the row exists."""
    return [-1, n_x, n - 1][turn % 3] if n_x < n else -1


# ================================================================================================================================
# (a) integer data, ==
# ================================================================================================================================
VARIANTS = [("dense", True, False), ("dense", False, True), ("stream", True, False), ("sparse", False, False), ("sparse", False, True),
            ("linear", False, True), ("linear-sp", False, True)]


@pytest.mark.parametrize("form,qw,ball", VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("n", ROWS)
def test_c_jac_and_hessian_diagonal_are_exact(dev_ctx, n, form, qw, ball):
    """Every storage form (with the common quadratic term where the class takes one, with the ball elsewhere) at every row count of ROWS
    -- odd and even, one row either side of a 64-row round and of a 512-row vector tile -- and every n_x edge; the slack row moves
    through {-1, n_x, n - 1}.  m_lin = 5: one-pass c! for the dense forms."""
    S = System(dev_ctx, form, n, 5, 100 * n + len(form), qw=qw, ball=ball)
    S.check_limits()
    for t, n_x in enumerate(nx_edges(n)):
        S.check(n_x, slack_for(n, n_x, t) if ball else -1)


ONEPASS_M = [4, 5, 16, 17, 32, 33, 64, 65, 96, 97, 125, 128, 129, 132, 133, 192, 193, 256, 257, 385, 513, 769, 1024]
GEMV_NT_M = [1, 2, 3, 1025]


@pytest.mark.parametrize("m", GEMV_NT_M + ONEPASS_M)
def test_c_through_every_tile_class_and_through_gemv_nt(dev_ctx, m):
    """c! of the dense class with kinds and the quadratic term at n = 130 (two 64-row rounds and a ragged one of 2; in the wide form eight
    16-row rounds and one of 2): m_lin of ONEPASS_M reaches each LF_OP tile class of run_onepass, narrow and wide, and one column either
    side of its upper edge; m_lin = 1, 2, 3 and 1025 lie outside the one-pass kernel and take run_gemv_nt.  In a second context with the
    one-pass kernels switched off (lfpsqp_ctx_set_onepass(-1), what the environment variable LFPSQP_ONEPASS=-1 sets) every width takes
    run_gemv_nt.  Both == the int64 reference, hence each other.  slack_row points at a row in [n_x, n): without a ball it means
    nothing."""
    ctx = dev_ctx
    n, n_x = 130, 77
    S = System(ctx, "dense", n, m, 31 * m, qw=True)
    S.check_limits()
    S.check(n_x, 100, what=("c",))
    S.check(n, -1, what=("c",))
    ctx2 = L.Context(0, ctx.L)
    try:
        ctx2.set_onepass(-1)
        S2 = System(ctx2, "dense", n, m, 31 * m, qw=True)
        S2.check(n_x, 100, what=("c",))
        S2.check(0, -1, what=("c",))
        del S2
    finally:
        ctx2.close()


@pytest.mark.parametrize("qw", [False, True])
@pytest.mark.parametrize("m", [1, 15, 16, 17, 31, 33])
def test_jac_column_blocks(dev_ctx, m, qw):
    """ew_jac_kernel takes kEwJacCols = 16 columns per workgroup: m_lin one column either side of one and of two blocks, with and without
    the quadratic term, n = 1027 (two 512-row blocks and one of 3 rows, odd): Jct[:, j] == phi'(x) .* A[:, j] + 2 qw_j x [i < n_x] entry by
    entry, the two spare columns of the caller's Jct keep their POISON.  The streamed form at the same widths: rs and u compared directly."""
    S = System(dev_ctx, "dense", 1027, m, 7 * m + qw, qw=qw)
    S.check_limits()
    for n_x in (600, 601):
        S.check(n_x)
    S = System(dev_ctx, "stream", 1027, m, 7 * m + qw, qw=qw)
    S.check(601)


@pytest.mark.parametrize("form,m", [("linear", 0), ("linear", 1), ("linear", 5), ("linear-sp", 1), ("linear-sp", 5), ("dense", 5), ("sparse", 5)])
@pytest.mark.parametrize("n", [130, 131])
def test_ball_and_slack(dev_ctx, n, form, m):
    """c[m_lin] == sum_{i<n_x} x_i^2 - x[slack_row] - R2, the ball column == [2x; -1 at slack_row; 0 elsewhere], hess_diag adds 2 lam[m_lin]
    below n_x only: slack_row in {-1, n_x, n - 1} with n_x = 64, 65 (the slack on an even and on an odd row, at a round edge) and n - 1 odd
    (n = 130) and even (n = 131).  The linear class with m_lin = 0, 1, 5, without and with Jsp, and the nonlinear class with a kind."""
    S = System(dev_ctx, form, n, m, 1000 * n + m, ball=True)
    S.check_limits()
    for n_x in (64, 65):
        for slack in (-1, n_x, n - 1):
            S.check(n_x, slack)
    S.check(n, -1)


@pytest.mark.parametrize("form", ["dense", "stream"])
@pytest.mark.parametrize("m", [3, 5, 133])
def test_quadratic_term_without_a_ball_ignores_slack_row(dev_ctx, form, m):
    """Sphere form: c_j == A'phi(x) + qw_j sum_{i<n_x} x_i^2 - b_j with n_x < n, whatever slack_row holds (include/lfpsqp_hip.h: slack_row means
    something with has_ball only) -- on the one-pass path (m_lin = 5, 133), on run_gemv_nt (m_lin = 3), with the one-pass kernels off, and
    from jac!'s own evaluation; with kinds and (kh = 0) with phi the identity, as the sphere system has it."""
    ctx = dev_ctx
    n, n_x = 130, 77
    for mode in (0, -1):
        ctx.set_onepass(mode)
        try:
            for kh in (None, np.zeros(n)):
                S = System(ctx, form, n, m, 5 * m, qw=True, kh=kh)
                S.check_limits()
                for slack in (-1, n_x, 100, n - 1):
                    S.check(n_x, slack, what=("c", "jac"))
        finally:
            ctx.set_onepass(0)


def test_hessian_diagonal_noop_and_alias(dev_ctx):
    """kind == NULL and cq == 0 (the linear class without a ball): hx keeps its bits, -0.0 and NaN included.  hx aliased to x is an argument
    error, for every class."""
    ctx = dev_ctx
    n = 131
    S = System(ctx, "linear", n, 5, 3)
    odd = np.concatenate([S.h0, np.full(PAD, POISON)])
    odd[:4] = [-0.0, np.nan, np.inf, 5e-324]
    S.hx.upload(odd)
    S.cons.hess_diag_(S.hx, S.x, S.lam)
    assert np.array_equal(bits(S.hx.download()), bits(odd))
    for form, kw in (("linear", dict(ball=True)), ("dense", dict(qw=True)), ("sparse", {}), ("stream", {})):
        S = System(ctx, form, n, 5, 4, **kw)
        with pytest.raises(L.LfpsqpError):
            S.cons.hess_diag_(S.x, S.x, S.lam)
        S.check(n)                                                         # (and the context is still usable)


SPOTS_N, SPOTS_NX = 1025, 700
SPOTS = [0, 63, 64, 511, 512, SPOTS_NX - 1, SPOTS_NX, SPOTS_N - 1]


@pytest.mark.parametrize("form,qw,ball", [("dense", True, False), ("stream", True, False), ("sparse", False, True), ("linear", False, True),
                                          ("linear-sp", False, True)], ids=lambda v: str(v))
@pytest.mark.parametrize("p", SPOTS)
def test_single_large_entry(dev_ctx, p, form, qw, ball):
    """A single 2^20 in A (row p, column 2) and in x (row p) on top of the small integers, p at the first and the last row, either side of
    n_x and at the 64-row and 512-row edges: a row counted twice, dropped or taken from the neighbouring lane shows as a difference of
    2^20 or more.  The sums stay exactly representable (checked in reference()): at most 5 * 2^40 + small."""
    n, m = SPOTS_N, 5
    seed = 900 + p
    r, c = sparse_pattern(seed + 11, n, m)
    Ah = np.zeros((n, m))
    Ah[r, c] = nonzero_ints(seed + 12, len(r), LIM_A)
    if form in ("dense", "stream", "linear"):
        Ah = ints(seed, (n, m), LIM_A)
    Ah[p, 2] = BIG
    xh = ints(seed + 1, n, LIM_X)
    xh[p] = BIG
    kh = np.random.default_rng(seed).choice([0.0, 2.0], n)
    kh[p] = 0.0                                                            # (t^2 of 2^20 times 2^20 would leave the exact range)
    S = System(dev_ctx, form, n, m, seed, qw=qw, ball=ball, Ah=Ah, xh=xh, kh=None if form.startswith("linear") else kh)
    slack = -1 if not ball else (p if p >= SPOTS_NX else n - 2)
    S.check(SPOTS_NX, slack)


# ================================================================================================================================
# (b) the sin kind
# ================================================================================================================================
# Worst error of the device's sin / cos over sin_args() against the correctly rounded mpmath value, in ulps of that value (FINDINGS.md 17):
#   CPU emulator (the host's libm)  sin 0.5000  cos 0.5009     MI355X (the device library)  not measured yet: no device was available
# S_ULP is the next whole ulp above the worst of them: a device value v~ of sin / cos differs from the true one v by at most S_ULP * ulp(v),
# where ulp(v) = 2^(floor(log2 |v|) - 52) <= 2 u |v| is the spacing of binary64 at v -- the unit the figures were measured in.
S_ULP = 1
S_ULP_MAX = 4                                    # beyond that something other than the library's rounding is wrong: fail outright


def sin_args(seed, n):
    """|x| from 2^-30 to 2^20, both signs; 0.0, -0.0; the binary64 neighbours of k pi / 2 for a few k up to 10^5."""
    rng = np.random.default_rng(seed)
    x = np.ldexp(rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n), rng.integers(-30, 20, n))
    near = [float(k * mpmath.pi / 2) for k in (1, 2, 3, 4, 5, 7, 22, 355, 1000, 51819, 99999, 100000)]
    near = np.array(near + [-v for v in near] + [np.nextafter(v, 0.0) for v in near[:4]])
    x[:2] = [0.0, -0.0]
    x[2:2 + len(near)] = near[:max(0, n - 2)]
    x[-1] = BIG
    return x


def mp_phi(kind, x, order):
    """phi, phi', phi'' of one variable in mpmath (exact for kinds 0 and 2)."""
    t = mpmath.mpf(float(x))
    if kind == 0:
        return (t, mpmath.mpf(1), mpmath.mpf(0))[order]
    if kind == 1:
        return (mpmath.sin(t), mpmath.cos(t), -mpmath.sin(t))[order]
    return (t * t, 2 * t, mpmath.mpf(2))[order]


def ulp_error(got, exact):
    """|got - exact| in ulps of the correctly rounded value of `exact` (an mpf); 0 when both are the same zero."""
    r = float(exact)
    if r == 0.0:                                                           # (mpmath has no signed zero: the caller looks at the sign)
        return 0.0 if got == 0.0 else math.inf
    return float(abs(mpmath.mpf(float(got)) - exact) / mpmath.mpf(ulp(r)))


@functools.lru_cache(maxsize=4)
def _sin_case(n, m, sparse):
    """(A, kind, x, qw, b, lam, h0) and the mpmath values phi, phi', phi'' per row."""
    seed = 7 * n + m
    rng = np.random.default_rng(seed)
    if sparse:
        r, c = sparse_pattern(seed, n, m)
        Ah = np.zeros((n, m))
        Ah[r, c] = short_reals(seed + 1, len(r), -8, 8)
    else:
        Ah = short_reals(seed + 1, n * m, -8, 8).reshape(n, m)
    kh = rng.integers(0, 3, n).astype(np.float64)
    kh[:40] = 1.0                                                          # (the hand-picked arguments all go through sin / cos)
    xh = sin_args(seed + 2, n)
    qh = nonzero_ints(seed + 3, m, LIM_S)
    bh = short_reals(seed + 4, m, -4, 4)
    lam = ints(seed + 5, m, LIM_S)
    h0 = short_reals(seed + 6, n, -4, 4)
    P = [[mp_phi(int(k), t, o) for k, t in zip(kh, xh)] for o in range(3)]
    for v in (Ah, kh, xh, qh, bh, lam, h0):
        v.setflags(write=False)
    return np.asfortranarray(Ah), kh, xh, qh, bh, lam, h0, P


def test_device_sin_and_cos_in_ulps(dev_ctx):
    """The device's own sin and cos, isolated: rs of the streamed form after jac! is cos(x) entry by entry, work of the sparse form after c!
    is sin(x).  Against the correctly rounded mpmath values: at most S_ULP ulps (the measured allowance the bounds below use), and never
    above 4.  The worst figures are printed (pytest -s) for FINDINGS.md."""
    ctx = dev_ctx
    n, m = 1025, 3
    xh = sin_args(5, n)
    A = ctx.matrix(n, m, ints(1, (n, m), LIM_A))
    x, kind = padded(ctx, xh, np.nan), padded(ctx, np.ones(n), 1.0)
    cs = L.ElementwiseConstraints(ctx, A, np.zeros(m), kind=kind, stream=True)
    cs.jac_(cs.Jct, np.zeros(m), x)
    cosd = cs.rs.download()
    r, c = sparse_pattern(3, n, m)
    Asp = L.SparseMatrix(ctx, n, m, r, c, nonzero_ints(4, len(r), LIM_A))
    cp = L.ElementwiseConstraints(ctx, Asp, np.zeros(m), kind=kind)
    cp.c_(np.zeros(m), x)
    sind = cp.work.download()[:n]
    es = [ulp_error(sind[i], mpmath.sin(mpmath.mpf(float(xh[i])))) for i in range(n)]
    ec = [ulp_error(cosd[i], mpmath.cos(mpmath.mpf(float(xh[i])))) for i in range(n)]
    ws, wc = int(np.argmax(es)), int(np.argmax(ec))
    print(f"\n[sin/cos ulp] {ctx.device_name}: sin worst {es[ws]:.4f} ulp at x = {float(xh[ws])!r}, cos worst {ec[wc]:.4f} ulp at x = {float(xh[wc])!r}; "
          f"above 0.5 ulp: sin {sum(e > 0.5 for e in es)}, cos {sum(e > 0.5 for e in ec)} of {n}")
    assert max(es[ws], ec[wc]) <= S_ULP_MAX, (es[ws], ec[wc])
    assert max(es[ws], ec[wc]) <= S_ULP, (es[ws], ec[wc])
    assert math.copysign(1.0, sind[1]) == -1.0 and sind[0] == 0.0 and cosd[0] == cosd[1] == 1.0      # sin(-0.0) = -0.0


def s_allow(v):
    """S_ULP ulps of the true value v (mpf) of a sin / cos."""
    r = float(v)
    return mpmath.mpf(S_ULP * ulp(r)) if r != 0.0 else mpmath.mpf(0)


def F(v):
    """A binary64 value as an mpf (exact).  The arithmetic below runs at 280 bits: its own roundings, 2^-280 relative, are 2^-220 of the
    smallest bound."""
    return mpmath.mpf(float(v))


def mp_gamma(k):
    g = gamma(k)
    return mpmath.mpf(g.numerator) / mpmath.mpf(g.denominator) * (1 + mpmath.mpf(2) ** -200)


@pytest.mark.parametrize("form", ["dense", "stream", "sparse"])
@pytest.mark.parametrize("n,m", [(513, 5), (1025, 33), (700, 130)])
def test_sin_kind_bounds(dev_ctx, n, m, form):
    """Mixed kinds {t, sin t, t^2} on real data: A and b with 26 significant bits, x of sin_args().  With s = S_ULP, u = 2^-53, v~ the device's
    sin / cos (|v~ - v| <= s ulp(v)), everything else from the roundings the kernels make:

      Jct_ij = fma(d_i, A_ij, qw_j * 2 x_i [i < n_x]),  d_i = phi'(x_i) (exact for kinds t, t^2; s ulps for cos):
          |Jct_ij - ref| <= s ulp(cos x_i) |A_ij| + u |2 qw_j x_i| (the qw product's rounding) + u |ref|              (the fma's one rounding)
          -- written with |ref| + the first two terms on the right, since the rounding acts on the computed sum;
      hx_i = h0_i + (phi''_i * (A lam)_i + cq [i < n_x]):  (A lam)_i summed over m_lin terms in any order, then a product and two sums;
          |hx_i - ref| <= (s ulp(phi''_i) (1 + gamma_{m+3}) + gamma_{m+3} |phi''_i|) sum_j |A_ij lam_j| + gamma_2 |cq| + u |h0_i|;
      c_j: |c_j - ref_j| <= (s' + gamma_{n+2}) sum_i |A_ij| |phi(x_i)| + u |b_j| with s' |phi_i| standing for s ulp(phi_i) on the sin rows, plus, with
          the quadratic term, gamma_{n+2} |qw_j| sum_{i<n_x} x_i^2 (its partial sums, the fma) -- the a-priori bound of a sum in any order.

    The true values are formed in mpmath at 280 bits from the binary64 inputs."""
    ctx = dev_ctx
    sparse = form == "sparse"
    Ah, kh, xh, qh, bh, lam, h0, P = _sin_case(n, m, sparse)
    qw = form == "dense"
    n_x = n - 101
    x, kind = padded(ctx, xh, np.nan), padded(ctx, kh, 1.0)
    if sparse:
        r, c = np.nonzero(Ah)
        A = L.SparseMatrix(ctx, n, m, r, c, Ah[r, c])
    else:
        A = ctx.matrix(n, m, Ah)
    cons = L.ElementwiseConstraints(ctx, A, bh, kind=kind, qw=qh if qw else None, n_x=n_x, stream=(form == "stream") if not sparse else None)
    cv, cvj = np.zeros(m), np.zeros(m)
    cons.c_(cv, x)
    cons.jac_(cons.Jct, cvj, x)
    assert np.array_equal(bits(cv), bits(cvj))
    Jd = cons.Jct.download()
    hx = padded(ctx, h0, POISON)
    cons.hess_diag_(hx, x, lam)
    hd = hx.download()
    assert np.all(hd[n:] == POISON)
    u, zero = mpmath.mpf(U), mpmath.mpf(0)
    sinrow = kh == 1.0
    Fx = [F(t) for t in xh]
    Fphi = P
    allow = [[s_allow(P[o][i]) if sinrow[i] else zero for i in range(n)] for o in range(3)]
    x2 = mpmath.fsum(Fx[i] * Fx[i] for i in range(n_x))
    cq = 2 * mpmath.fsum(F(qh[j]) * F(lam[j]) for j in range(m)) if qw else zero
    nz = [np.nonzero(Ah[:, j])[0] for j in range(m)] if sparse else [range(n)] * m
    g_n, g_m, g_2 = mp_gamma(n + 2), mp_gamma(m + 3), mp_gamma(2)
    FA = [[F(Ah[i, j]) for j in range(m)] for i in range(n)]
    # c!
    for j in range(m):
        ref = mpmath.fsum(FA[i][j] * Fphi[0][i] for i in nz[j]) - F(bh[j])
        bound = mpmath.fsum(abs(FA[i][j]) * (allow[0][i] + g_n * abs(Fphi[0][i])) for i in nz[j]) + u * abs(F(bh[j]))
        if qw:
            ref += F(qh[j]) * x2
            bound += g_n * abs(F(qh[j])) * x2
        assert abs(F(cv[j]) - ref) <= bound, (form, n, m, j, cv[j], float(ref), float(bound))
    # jac!
    for j in range(m):
        fq = 2 * F(qh[j]) if qw else zero
        for i in nz[j]:
            ref = Fphi[1][i] * FA[i][j] + (fq * Fx[i] if i < n_x else 0)
            first = allow[1][i] * abs(FA[i][j]) + (u * abs(fq * Fx[i]) if i < n_x else 0)
            bound = first + u * (abs(ref) + first)
            assert abs(F(Jd[i, j]) - ref) <= bound, (form, n, m, i, j, Jd[i, j], float(ref), float(bound), kh[i], xh[i])
    if sparse:
        assert np.array_equal(bits(cons.Jsp.to_dense().download()), bits(Jd[:, :m]))
        assert np.all(Jd[Ah == 0.0] == 0.0)
    # hess_diag
    Fl = [F(v) for v in lam]
    for i in range(n):
        row = [FA[i][j] * Fl[j] for j in range(m)]
        Si = mpmath.fsum(abs(t) for t in row)
        ref = F(h0[i]) + Fphi[2][i] * mpmath.fsum(row) + (cq if i < n_x else 0)
        bound = (allow[2][i] * (1 + g_m) + g_m * abs(Fphi[2][i])) * Si + (g_2 * abs(cq) if i < n_x else 0) + u * abs(F(h0[i]))
        assert abs(F(hd[i]) - ref) <= bound, (form, n, m, i, hd[i], float(ref), float(bound))
    assert np.array_equal(bits(x.download()[:n]), bits(xh))


# ================================================================================================================================
# (c) the sparse products
# ================================================================================================================================
SPMV_T_CONFIGS = [(16400, [16385, 0, 8193]),      # the longest column first, an empty one between two long ones; 3 and 2 chunks
                  (16400, [8191, 8192, 16385]),   # the longest last; one nonzero short of a chunk, a whole chunk
                  (4200, [2047, 4097, 2049]),     # one short of an unrolled step of 8 x 256, two steps and one, one step and one
                  (2100, [2048, 255, 256]),       # exactly one unrolled step; a wave short of / exactly one pass of the tail loop
                  (300, [257, 1, 0]),
                  (16400, [16385]),               # m == 1
                  (2100, [2048]),
                  (9000, [0, 8192, 0])]


def column_rows(seed, n, counts):
    """Rows of each column: a sorted random subset of the n rows of the given size (at most len(counts) <= 3 nonzeros per row, some rows
    empty)."""
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(n, c, replace=False)) for c in counts]


def sp_from_columns(ctx, n, rows, vals):
    r = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    c = np.concatenate([np.full(len(rr), j) for j, rr in enumerate(rows)]) if rows else np.zeros(0, dtype=np.int64)
    v = np.concatenate(vals) if vals else np.zeros(0)
    p = np.random.default_rng(len(r)).permutation(len(r))                  # (triplets in no particular order)
    return L.SparseMatrix(ctx, n, len(rows), r[p], c[p], v[p])


@pytest.mark.parametrize("n,counts", SPMV_T_CONFIGS, ids=lambda v: str(v).replace(" ", ""))
def test_spmv_t_is_exact_at_every_column_length(dev_ctx, n, counts):
    """t = S'v with columns of exactly 0, 1, 255, 256, 257, 2047, 2048, 2049, 4097, 8191, 8192, 8193 and 16385 nonzeros: spmv_t_chunk_kernel takes
    8 x 256 = 2048 nonzeros per unrolled step and 256 per step of its tail loop, a column is cut into chunks of kSpChunk = 8192 that
    spmv_t_final_kernel adds up.  |values| <= 16, |v_i| <= 1024, integers: t == the int64 product, bit for bit.  v is longer than n with a NaN
    tail, t longer than m with a POISON tail that stays.  Then a single 2^20 in v at the row of a column's nonzero number 2047, 2048, 8191
    and 8192 (0-based: the last of an unrolled step / chunk and the first of the next)."""
    ctx = dev_ctx
    m = len(counts)
    rows = column_rows(n + m, n, counts)
    vals = [nonzero_ints(j + n, len(rr), LIM_A) for j, rr in enumerate(rows)]
    S = sp_from_columns(ctx, n, rows, vals)
    assert S.nnz == sum(counts) and S.ell_width <= 3
    vh = ints(n, n, 1024)
    v, t = padded(ctx, vh, np.nan), padded(ctx, np.zeros(m), POISON)

    def run(vh):
        v.upload(vh)
        t.upload(np.full(m, POISON))
        out = L.spmv_t(S, v, t).download()
        ref = np.array([int(i64(vals[j]) @ i64(vh[rows[j]])) for j in range(m)], dtype=np.int64)
        assert np.array_equal(out[:m], ref), (out[:m], ref)
        assert np.all(out[m:] == POISON)
    run(vh)
    for j in range(m):
        for k in (2047, 2048, 8191, 8192):
            if counts[j] > k:
                v2 = vh.copy()
                v2[rows[j][k]] = BIG
                run(v2)
    assert np.array_equal(bits(v.download()[n:]), bits(np.full(PAD, np.nan)))


@pytest.mark.parametrize("n", [129, 700])
@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 32, 256])
def test_spmv_n_is_exact_at_every_ell_width(dev_ctx, K, n):
    """y = alpha S t + beta y with the widest row holding K nonzeros (256: the widest lfpsqp_spmat_create accepts; 257 is refused), rows of
    every count below it and rows without any, n odd and even.  beta == 0 with a NaN-filled y (y is not read), alpha == 0, both general; y is
    longer than n and its tail stays; t aliased to y is an argument error."""
    ctx = dev_ctx
    m = K + 3
    rng = np.random.default_rng(K * n)
    D = np.zeros((n, m))
    for i in range(n):
        k = K if i == n // 2 else (0 if i % 7 == 3 else int(rng.integers(0, K + 1)))
        D[i, rng.choice(m, k, replace=False)] = nonzero_ints(i, k, LIM_A)
    r, c = np.nonzero(D)
    S = L.SparseMatrix(ctx, n, m, r, c, D[r, c])
    assert S.ell_width == K
    th, yh = ints(K, m, LIM_A), ints(K + 1, n, 1024)
    t, y = padded(ctx, th, np.nan), padded(ctx, yh, POISON)
    St = imatmul(i64(D), i64(th))
    for alpha, beta in ((1, 0), (-3, 0), (2, -3), (0, 2), (0, 0), (1, 1)):
        y.upload(np.full(n, np.nan) if beta == 0 else yh)
        out = L.spmv_n(S, t, y, alpha, beta).download()
        assert np.array_equal(out[:n], alpha * St + beta * i64(yh)), (alpha, beta)
        assert np.all(out[n:] == POISON)
    tt = ctx.vector(max(n, m) + PAD)
    with pytest.raises(L.LfpsqpError):
        L.spmv_n(S, tt, tt)
    if K == 256:
        with pytest.raises(L.LfpsqpError):
            L.SparseMatrix(ctx, 3, 257, np.ones(257, dtype=np.int64), np.arange(257), np.ones(257))


@pytest.mark.parametrize("n,counts", [(2100, [2048, 255, 256]), (9000, [0, 8193, 1])], ids=["2100", "9000"])
def test_rowscale_writes_both_storage_orders(dev_ctx, n, counts):
    """dst == src .* v in the ELL copy (read by spmv_n) and in the CSC copy (read by spmv_t and to_dense): all three == the int64 reference.
    v holds zeros and -0.0 (the signs of the zeros are compared through to_dense); a clone scaled twice holds src .* v2, not
    src .* v1 .* v2; src keeps its values."""
    ctx = dev_ctx
    m = len(counts)
    rows = column_rows(n, n, counts)
    vals = [nonzero_ints(j + 3, len(rr), LIM_A) for j, rr in enumerate(rows)]
    src = sp_from_columns(ctx, n, rows, vals)
    dst = src.clone()
    D = np.zeros((n, m))
    for j in range(m):
        D[rows[j], j] = vals[j]
    th, wh = ints(1, m, LIM_A), ints(2, n, LIM_A)
    t, w = ctx.vector(m, th), ctx.vector(n, wh)
    for seed in (5, 6):
        vh = ints(seed, n, LIM_A)
        vh[rows[0][:3] if counts[0] else rows[1][:3]] = [-0.0, 0.0, -0.0]
        v = padded(ctx, vh, np.nan)
        dst.rowscale_from(src, v)
        ref = np.zeros((n, m))
        for j in range(m):
            ref[rows[j], j] = vals[j] * vh[rows[j]]                        # (one exact product per entry: the signs of zero as IEEE has them)
        M = ctx.matrix(n, m + 1)
        M.upload(np.full((n, m + 1), POISON))
        dense = dst.to_dense(M).download()
        assert np.array_equal(bits(dense[:, :m]), bits(ref)), seed
        assert np.all(dense[:, m] == POISON)
        Ri = i64(ref)
        assert np.array_equal(L.spmv_t(dst, w, ctx.vector(m)).download(), imatmul(Ri.T, i64(wh))), seed       # the CSC copy
        assert np.array_equal(L.spmv_n(dst, t, ctx.vector(n)).download(), imatmul(Ri, i64(th))), seed         # the ELL copy
        assert np.array_equal(src.to_dense().download(), D)
        assert np.array_equal(L.spmv_n(src, t, ctx.vector(n)).download(), imatmul(i64(D), i64(th)))


def test_to_dense_duplicates_unsorted_and_spare_columns(dev_ctx):
    """Triplets in descending order with duplicates, one pair summing to zero: every position once, the cancelled one an explicit 0.0; the
    columns of M beyond S.m are left alone (include/lfpsqp_hip.h), the columns below it overwritten (zeros where S has nothing)."""
    ctx = dev_ctx
    n, m = 67, 4
    rows = np.array([66, 66, 40, 40, 40, 3, 3, 0], dtype=np.int64)
    cols = np.array([3, 0, 2, 2, 1, 3, 3, 0], dtype=np.int64)
    vals = np.array([5.0, -2.0, 7.0, -7.0, 1.0, 4.0, 6.0, 9.0])
    S = L.SparseMatrix(ctx, n, m, rows, cols, vals)
    assert S.nnz == 6 and S.ell_width == 2
    ref = np.zeros((n, m))
    ref[66, 3], ref[66, 0], ref[40, 1], ref[3, 3], ref[0, 0] = 5.0, -2.0, 1.0, 10.0, 9.0
    M = ctx.matrix(n, m + 2)
    M.upload(np.full((n, m + 2), POISON))
    out = S.to_dense(M).download()
    assert np.array_equal(bits(out[:, :m]), bits(ref))
    assert np.all(out[:, m:] == POISON)
    v, t = ctx.vector(n, np.arange(n)), ctx.vector(m)
    assert np.array_equal(L.spmv_t(S, v, t).download(), [-2.0 * 66, 40.0, 0.0, 5.0 * 66 + 30.0])


@pytest.mark.parametrize("n,counts", [(9000, [8193, 300, 2049])], ids=["9000"])
def test_spmv_t_error_bound_on_cancelling_data(dev_ctx, n, counts):
    """Values and v with 26 significant bits over 60 binades (every product exact), the second half of each column the negated first half
    in another order but for a remainder: the column sums cancel to a small fraction of sum |terms|.  |t_j - exact| <= gamma_k sum |terms|,
    k = the column's nonzeros + its chunks (each product fused into its sum: one rounding per term; the lanes' partial sums, the
    workgroup's reduction and the chunks add fewer roundings to any one term than there are terms).  The true value is math.fsum of the
    exact products."""
    ctx = dev_ctx
    m = len(counts)
    rows = column_rows(n + 1, n, counts)
    vh = short_reals(3, n, -20, 20)
    vals = []
    for j, rr in enumerate(rows):
        a = short_reals(10 + j, len(rr), -10, 10)
        h = len(rr) // 2
        prod = a[:h] * vh[rr[:h]]                                          # exact
        # the mirrored half: same magnitudes with the other sign, through a value that reproduces the product exactly where it can
        perm = np.random.default_rng(j).permutation(h)
        tgt = -prod[perm]
        b = tgt / vh[rr[h:2 * h]]
        b = np.ldexp(np.round(np.ldexp(np.frexp(b)[0], 26)), np.frexp(b)[1] - 26)       # 26 significant bits again
        a[h:2 * h] = b
        a[2 * h:] = np.ldexp(a[2 * h:], -60)                                # (an odd count's last term: far below the others)
        vals.append(a)
    S = sp_from_columns(ctx, n, rows, vals)
    out = L.spmv_t(S, ctx.vector(n, vh), ctx.vector(m)).download()
    for j in range(m):
        terms = vals[j] * vh[rows[j]]
        assert all(Fraction(float(a)) * Fraction(float(b)) == Fraction(float(p)) for a, b, p in zip(vals[j][::97], vh[rows[j]][::97], terms[::97]))
        exact, tot = fsum(terms), fsum(np.abs(terms))
        k = counts[j] + -(-counts[j] // 8192)
        assert abs(exact) < 1e-3 * tot                                     # (the data does cancel)
        assert abs(Fraction(float(out[j])) - Fraction(exact)) <= gamma(k) * Fraction(tot), (j, out[j], exact, tot)


@pytest.mark.parametrize("K", [3, 9, 32])
def test_spmv_n_error_bound_on_cancelling_data(dev_ctx, K):
    """y_i = sum of a row's K exact products, cancelling pairwise but for one: |y_i - exact| <= gamma_K sum |terms| (alpha = 1, beta = 0)."""
    ctx = dev_ctx
    n, m = 301, K + 2
    rng = np.random.default_rng(K)
    th = short_reals(K, m, -20, 20)
    D = np.zeros((n, m))
    for i in range(n):
        cols = rng.choice(m, K, replace=False)
        a = short_reals(1000 * K + i, K, -10, 10)
        for p in range(0, K - 1, 2):                                        # a_{p+1} t_{p+1} ~ -a_p t_p
            b = -a[p] * th[cols[p]] / th[cols[p + 1]]
            fr, ex = math.frexp(b)
            a[p + 1] = math.ldexp(round(math.ldexp(fr, 26)), ex - 26)
        D[i, cols] = a
    r, c = np.nonzero(D)
    S = L.SparseMatrix(ctx, n, m, r, c, D[r, c])
    out = L.spmv_n(S, ctx.vector(m, th), ctx.vector(n, np.full(n, np.nan))).download()
    for i in range(n):
        terms = D[i] * th                                                  # exact: 26 x 26 bits
        exact, tot = fsum(terms), fsum(np.abs(terms))
        assert abs(Fraction(float(out[i])) - Fraction(exact)) <= gamma(K) * Fraction(tot), (i, out[i], exact)


# ================================================================================================================================
# (d) GPU only: several rounds per workgroup
# ================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("m", [5, 128, 133, 260])
def test_c_with_several_rounds_per_workgroup(gpu_lib, m):
    """n = 70001 = 1093 rounds of 64 rows and one of 49 (wide form, m_lin = 260: 4375 rounds of 16 and one of 1).  The c! launch has at most two
    workgroups per CU (kEwWgPerCu): 512 on the 256 CUs of an MI355X, so a workgroup turns the round loop of onepass_kernel's eval_only form 2
    to 5 times in the narrow classes and 8 to 17 times in the wide one, the last round ragged -- which no small case does.  Integer data, ==
    the int64 reference; jac!'s own evaluation and the Hessian diagonal ride along."""
    ctx = L.Context(0, gpu_lib)
    try:
        assert "emulator" not in ctx.device_name
        n = 70001
        S = System(ctx, "dense", n, m, 13 * m, qw=True)
        S.check_limits()
        S.check(n - 7, 69999)
        S.check(n, -1, what=("c",))
    finally:
        ctx.close()
