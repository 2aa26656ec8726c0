"""pcg! fused on the device (lfpsqp_pcg, lfpsqp_pcg_pre: csrc/pcg.hip -- PInit, P1V / P1VS, P2E / P2ES, P3F, PPost3, PcgInnerE<ST> through
onepass_kernel, pcg_tmp_kernel, the sparse forms P1SparseF / P2SparseF, PrecS0V<ST>, PrecZE<ST>, PrecQE<ST>, PrecP3F, prec_small_kernel)
against exact and high-precision references of the reference's loop (src/retractions.jl:179-246).

The C entry points are called directly with `_capi.Basis` / `_capi.PcgPrecond`, so Dx, Dy, sx, sy, i11, i12, i22 and K are free inputs.

  (A) lfpsqp_pcg on integer data built so that alpha_1 = 2^-k: after one iteration x, r, p, z == an integer reference, after two
      iterations p, z == (they consume the sums u = J z and s = J r of the fused kernel) and x, r lie inside a derived allowance -- every
      tile class of run_onepass and one column either side, plain and stacked, one-pass and two-pass, sparse twin, staged stores;
  (B) lfpsqp_pcg_pre on integer data with mu = 4: first iteration ==; K' against K; sx, sy other than (1, 0); refusals;
  (C) K = 1, 2, 4 iterations on real data against the same statements in mpmath at 280 bits, inside K kappa gamma_{n+m+4};
  (D) a solve stopped by tol leaves the bits of the solve stopped by maxiter (the host queues launches ahead of the device-side stop);
      maxiter <= 0, NaN right-hand side, tol = Inf / NaN;
  (E) lfpsqp_pcg against the statement-by-statement loop on the device primitives.

The integer references hold every quantity as Python integers a with the value a * 2^-e (object arrays; the matrix products in int64,
guarded against overflow).  `dbl` asserts that what it hands to == is a binary64 number, `fits` that a sum's terms, in the unit the
reference holds them in, add up in absolute value to less than 2^53 -- then every partial sum in ANY order is exact, on any device."""
import ctypes as C
import math

import mpmath
import numpy as np
import pytest

import lfpsqp_jl_amd as L
from lfpsqp_jl_amd import _capi
from oracle import lfpsqp_ref as R
from tests.helpers import gamma, imatmul

ERR_ARG, ERR_UNSUPPORTED = -1, -5
MARK = 12345.0                                   # finite marker in p and z before a solve
ONEPASS_M = [4, 5, 16, 17, 32, 33, 64, 65, 96, 97, 125, 128, 129, 132, 133, 192, 193, 256, 257, 385, 513, 769, 1024]
ALL_M = [0, 1, 3, 1025] + ONEPASS_M              # (0, 1, 3, 1025: outside the one-pass kernel -- the two-pass form)
SPARE = 2                                        # columns of Jct beyond ncols, NaN-filled


def is_emu(ctx):
    return "emulator" in ctx.device_name


# ================================================================================================================================
# the operator on the device
# ================================================================================================================================
class Op:
    """J' in the lfpsqp_basis form on `ctx`: plain (D is None) or stacked with D = (Dx, Dy, sx, sy); optionally with the sparse twin."""

    def __init__(self, ctx, Jt, D=None, sparse=False):
        self.ctx = ctx
        self.N, self.m = Jt.shape
        self.st = D is not None
        self.hs = int(ctx.L.lfpsqp_half_stride(self.N)) if self.st else 0
        self.nv = self.hs + self.N if self.st else self.N
        full = np.full((self.N, self.m + SPARE), np.nan, order="F")
        full[:, :self.m] = Jt
        self.Z = ctx.matrix(self.N, self.m + SPARE, full)
        self.D = [ctx.vector(self.N, d) for d in D] if self.st else [None] * 4
        self.tmp_w = ctx.vector(self.N) if self.st else None
        self.tmp_m = ctx.vector(max(self.m, 1))
        self.S = None
        if sparse:
            rows, cols = np.nonzero(Jt)
            self.S = L.SparseMatrix(ctx, self.N, self.m, rows, cols, np.asarray(Jt)[rows, cols])
        h = lambda v: v.h if v is not None else None
        self.basis = _capi.Basis(self.Z.h, self.m, h(self.D[0]), h(self.D[1]), h(self.D[2]), h(self.D[3]), None, None, h(self.S), None)

    def pack(self, v):
        """logical vector (N, or 2N = [x; y]) -> device layout (the gap between the halves zero)."""
        v = np.asarray(v, dtype=np.float64)
        if not self.st:
            return v.copy()
        out = np.zeros(self.nv)
        out[:self.N] = v[:self.N]
        out[self.hs:] = v[self.N:]
        return out

    def unpack(self, full, gap=True):
        """device layout -> logical vector; the gap must be exactly zero."""
        if not self.st:
            return full
        assert not gap or not full[self.N:self.hs].any(), "the gap between the halves of a stacked vector is not zero"
        return np.concatenate([full[:self.N], full[self.hs:]])

    def solve(self, mu, x0, r0, tol, maxiter, pre=None, gap=True):
        """lfpsqp_pcg (pre = None) or lfpsqp_pcg_pre (pre = (K, i11, i12, i22)) -> (rc, flag, iters, {x, r, p, z[, q]}), logical vectors.
        p holds the marker everywhere, z (and q) on its halves."""
        ctx = self.ctx
        mark = self.pack(np.full(2 * self.N if self.st else self.N, MARK))
        v = {"x": ctx.vector(self.nv, self.pack(x0)), "r": ctx.vector(self.nv, self.pack(r0)), "p": ctx.vector(self.nv, np.full(self.nv, MARK)),
             "z": ctx.vector(self.nv, mark)}
        flag, iters = C.c_int(-7), _capi.c_i64(-7)
        if pre is None:
            rc = ctx.L.lfpsqp_pcg(ctx.h, float(mu), C.byref(self.basis), v["x"].h, v["r"].h, v["p"].h, v["z"].h,
                                  self.tmp_w.h if self.st else None, self.tmp_m.h, float(tol), int(maxiter), C.byref(flag), C.byref(iters))
        else:
            K, i11, i12, i22 = pre
            K = np.asfortranarray(K, dtype=np.float64)
            v["q"] = ctx.vector(self.nv, mark)
            ii = [ctx.vector(self.N, a) for a in (i11, i12, i22)] if i11 is not None else [None] * 3
            h = lambda a: a.h if a is not None else None
            pc = _capi.PcgPrecond(K.ctypes.data, h(ii[0]), h(ii[1]), h(ii[2]), v["q"].h)
            rc = ctx.L.lfpsqp_pcg_pre(ctx.h, float(mu), C.byref(self.basis), C.byref(pc), v["x"].h, v["r"].h, v["p"].h, v["z"].h,
                                      float(tol), int(maxiter), C.byref(flag), C.byref(iters))
        out = {k: self.unpack(a.download(), gap) if rc == 0 else a.download() for k, a in v.items()}
        return rc, flag.value, iters.value, out


def twopass_ctx(ctx):
    c2 = L.Context(0, ctx.L)
    c2.set_onepass(-1)
    return c2


# ================================================================================================================================
# integer arithmetic: a * 2^-e
# ================================================================================================================================
def obj(a):
    return np.array([int(v) for v in np.asarray(a).ravel().tolist()], dtype=object)


def dbl(a, e=0):
    """The integers a * 2^-e as binary64 -- asserted to BE binary64 numbers."""
    a = np.atleast_1d(np.asarray(a, dtype=object))
    f = np.array([float(v) for v in a.tolist()], dtype=np.float64)
    assert all(int(x) == v for x, v in zip(f.tolist(), a.tolist())), "a reference value is not a binary64 number"
    return np.ldexp(f, -e)


def fits(abs_sum):
    """abs_sum: per output entry, the absolute values of a sum's terms added up (integers in the common unit)."""
    return max([int(v) for v in np.atleast_1d(abs_sum).tolist()], default=0) < 2 ** 53


def exact_ints(a):
    """binary64 numbers as (integers, e): a = integers * 2^e."""
    assert np.isfinite(a).all()
    m, e = np.frexp(a)
    e = e.astype(np.int64) - 53
    emin = int(e.min())
    return obj(np.ldexp(m, 53).astype(np.int64)) * 2 ** obj(e - emin), emin


def step_error(dev, frac, terms):
    """`dev` against base + alpha * d = num / den (frac = (num, alpha * d * den, den), integers) in exact arithmetic: the largest ratio of
    |dev - num / den| to the allowance (u + gamma_{terms + 2}) |alpha d| + u |num / den|  (u = 2^-53, gamma_k = k u / (1 - k u)).
    alpha = rho / p'z carries the gamma_{terms} of the dot product and two roundings, the update one more of its product and one of its sum."""
    num, step, den = frac
    X, e = exact_ints(dev)
    s, t = 2 ** max(-e, 0), 2 ** max(e, 0)
    kk, u1 = terms + 2, 2 ** 53
    lhs = abs(X * t * den - num * s) * u1 * (u1 - kk)
    rhs = (((u1 - kk) + kk * u1) * abs(step) + (u1 - kk) * abs(num)) * s
    assert all(l == 0 for l, r in zip(lhs.tolist(), rhs.tolist()) if r == 0)
    return max((l / r for l, r in zip(lhs.tolist(), rhs.tolist()) if r != 0), default=0.0)


class NotExact(Exception):
    pass


def need(ok):
    if not ok:
        raise NotExact()


def imul(A, v):
    """int64 matrix (entries in {-1, 0, 1}) times a vector of Python integers, and the same with absolute values."""
    if A.shape[1] == 0:
        return np.zeros(A.shape[0], dtype=object), np.zeros(A.shape[0], dtype=object)
    need(max(abs(int(x)) for x in v.tolist()) * max(A.shape[1], 1) < 2 ** 62)          # (int64 does not overflow)
    v64 = v.astype(np.int64)
    return imatmul(A, v64).astype(object), imatmul(np.abs(A), np.abs(v64)).astype(object)


class IntOp:
    """The operator on integers: J = [diag Dx, diag Dy; Z' diag sx, Z' diag sy] (stacked) or Z' (plain), Z with entries in {-1, 0, 1}."""

    def __init__(self, Z, D=None):
        self.Z = np.ascontiguousarray(Z, dtype=np.int64)
        self.Zt = np.ascontiguousarray(self.Z.T)
        self.N, self.m = Z.shape
        self.D = [obj(d) for d in D] if D is not None else None

    def J(self, p):
        """-> (w, t, ok): diagonal block (None when plain), Z block, whether every sum is exact in any order."""
        if self.D is None:
            t, ta = imul(self.Zt, p)
            return None, t, fits(ta)
        Dx, Dy, sx, sy = self.D
        px, py = p[:self.N], p[self.N:]
        w = Dx * px + Dy * py
        v = sx * px + sy * py
        t, ta = imul(self.Zt, v)
        return w, t, fits(ta) and fits(abs(Dx * px) + abs(Dy * py)) and fits(abs(sx * px) + abs(sy * py))

    def Jt(self, w, t):
        """J'[w; t] -> (z, |terms| summed)."""
        a, aa = imul(self.Z, t)
        if self.D is None:
            return a, aa
        Dx, Dy, sx, sy = self.D
        return (np.concatenate([Dx * w + sx * a, Dy * w + sy * a]),
                np.concatenate([abs(Dx * w) + abs(sx) * aa, abs(Dy * w) + abs(sy) * aa]))


def tern(rng, shape, density):
    a = rng.integers(0, 2, size=shape) * 2 - 1
    if density < 1.0:
        a[rng.random(size=shape) >= density] = 0
    else:
        a[rng.random(size=shape) < 0.25] = 0
    return a.astype(np.int64)


def capped_rows(rng, Z, kmax):
    """At most kmax nonzeros per row (the sparse twin's ELL width)."""
    Z = Z.copy()
    for i in range(Z.shape[0]):
        nz = np.flatnonzero(Z[i])
        if len(nz) > kmax:
            Z[i, rng.choice(nz, len(nz) - kmax, replace=False)] = 0
    return Z


# ================================================================================================================================
# (A) lfpsqp_pcg: two exact iterations
# ================================================================================================================================
def two_iterations(Z, D, r0, x0, q):
    """The statements of pcg! (src/retractions.jl:202-238) for two iterations in integers.  r0 has 2^q entries +-1, mu = 2^k - T / 2^q with
    T = |J r0|^2, so p_1'z_1 = 2^(q + k) and alpha_1 = 2^-k.  Raises NotExact when some sum of the device's would not be exact in every order."""
    op = IntOp(Z, D)
    r0, x0 = obj(r0), obj(x0)
    assert sum(abs(v) for v in r0.tolist()) == 2 ** q and set(r0.tolist()) <= {-1, 0, 1}
    # -- iteration 1: p = r0, tmp = J p, z = J'tmp + mu p
    w1, t1, ok = op.J(r0)
    need(ok)
    T = int(sum(v * v for v in t1.tolist())) + (int(sum(v * v for v in w1.tolist())) if w1 is not None else 0)
    k = max(T.bit_length() - q, 0)
    mu_n = 2 ** (k + q) - T                                      # mu = mu_n * 2^-q
    assert mu_n > 0
    jj, ja = op.Jt(w1, t1)
    z1 = jj * 2 ** q + mu_n * r0                                 # e = q
    need(fits(ja * 2 ** q + mu_n * abs(r0)))
    pz = int(np.dot(r0, z1))
    assert pz == 2 ** (q + k) * 2 ** q                           # p'z = 2^(q + k): alpha = 2^q / 2^(q + k)
    x1 = x0 * 2 ** k + r0                                        # e = k
    r1 = r0 * 2 ** (q + k) - z1                                  # e = q + k
    rr1 = int(np.dot(r1, r1))                                    # e = 2 (q + k)
    need(rr1 < 2 ** 53)
    one = {"mu": math.ldexp(mu_n, -q), "x": dbl(x1, k), "r": dbl(r1, q + k), "p": dbl(r0), "z": dbl(z1, q)}
    if rr1 == 0:                                                 # (a one-dimensional solve, or m = 0: converged; the loop ends on norm_res > tol)
        return one, None
    # -- iteration 2: beta = rr1 / 2^q ; p = r1 + beta p ; tmp = (s - alpha u) + beta tmp with u = J z1, s = J r0
    eb = 2 * (q + k) + q                                         # beta = rr1 * 2^-eb
    p2 = r1 * 2 ** (eb - (q + k)) + rr1 * r0                     # e = eb
    _, u, ok = op.J(z1)                                          # e = q
    need(ok)
    jr = t1 * 2 ** (q + k) - u                                   # J r1 = s - alpha u, e = q + k
    t2 = jr * 2 ** (eb - (q + k)) + rr1 * t1                     # e = eb
    w2, t2d, ok = op.J(p2)
    need(ok)
    assert all(a == b for a, b in zip(t2.tolist(), t2d.tolist()))        # (the recurrence IS J p2)
    dbl(u, q), dbl(jr, q + k), dbl(t2, eb)
    jj, ja = op.Jt(w2, t2)
    z2 = jj * 2 ** q + mu_n * p2                                 # e = eb + q
    need(fits(ja * 2 ** q + mu_n * abs(p2)))
    pz2 = int(np.dot(p2, z2))                                    # e = 2 eb + q
    assert pz2 > 0
    two = {"p": dbl(p2, eb), "z": dbl(z2, eb + q)}
    # x2 = x1 + alpha2 p2 and r2 = r1 - alpha2 z2 with alpha2 = rr1 / (p2'z2) = rr1 * 2^sh / pz2, as fractions num / den over one denominator
    sh = 2 * eb + q - 2 * (q + k)
    two["x_frac"] = (x1 * 2 ** (eb - k) * pz2 + rr1 * 2 ** sh * p2, rr1 * 2 ** sh * p2, pz2 * 2 ** eb)
    two["r_frac"] = (r1 * 2 ** (eb - k) * pz2 - rr1 * 2 ** sh * z2, rr1 * 2 ** sh * z2, pz2 * 2 ** (eb + q))
    two["terms"] = len(r0)
    return one, two


def case_A(seed, n, m, stacked, kmax=None, densities=(1.0, 0.25, 0.1, 0.05)):
    """Data for (A), thinned (fewer +-1 in r0, then a sparser Z) until the integer reference is exact in every summation order."""
    total = 2 * n if stacked else n
    qmax = min(4, int(math.log2(total)))
    qmin = 1 if (stacked and total >= 2) else 0
    for density in densities:
        for q in range(qmax, qmin - 1, -1):
            rng = np.random.default_rng([seed, n, m, int(stacked), q, int(density * 100)])
            Z = tern(rng, (n, m), density)
            if kmax is not None:
                Z = capped_rows(rng, Z, kmax)
            D = [rng.integers(-2, 3, n) for _ in range(4)] if stacked else None
            r0 = np.zeros(total, dtype=np.int64)
            if stacked:                                          # spans both halves
                pos = np.concatenate([rng.choice(n, 2 ** q // 2, replace=False), n + rng.choice(n, 2 ** q - 2 ** q // 2, replace=False)])
            else:
                pos = rng.choice(total, 2 ** q, replace=False)
            r0[pos] = rng.integers(0, 2, len(pos)) * 2 - 1
            x0 = rng.integers(-2, 3, total)
            try:
                one, two = two_iterations(Z, D, r0, x0, q)
            except NotExact:
                continue
            if two is None and n >= 2 and m >= 1:                # (r0 happened to be an eigenvector: no second iteration to check)
                continue
            return Z, D, r0, x0, one, two
    raise AssertionError("no exactly representable case found")


def check_A(op, r0, x0, one, two, tag=""):
    rc, flag, it, o = op.solve(one["mu"], x0, r0, 0.0, 1)
    assert (rc, flag, it) == (0, 1, 1), (tag, rc, flag, it)
    for k in ("x", "r", "p", "z"):
        np.testing.assert_array_equal(o[k], one[k], err_msg=f"{tag} iteration 1: {k}")
    rc, flag, it, o = op.solve(one["mu"], x0, r0, 0.0, 2)
    if two is None:                                              # r_1 = 0 exactly: 0 > tol = 0 is false, the second iteration is not run
        assert (rc, flag, it) == (0, 0, 1), (tag, rc, flag, it)
        for k in ("x", "r", "p", "z"):
            np.testing.assert_array_equal(o[k], one[k], err_msg=f"{tag} stopped after iteration 1: {k}")
        return 0.0
    assert (rc, flag, it) == (0, 1, 2), (tag, rc, flag, it)
    for k in ("p", "z"):
        np.testing.assert_array_equal(o[k], two[k], err_msg=f"{tag} iteration 2: {k}")
    worst = 0.0
    for k in ("x", "r"):
        ratio = step_error(o[k], two[k + "_frac"], two["terms"])
        assert ratio <= 1.0, (tag, k, ratio)
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("stacked", [False, True], ids=["plain", "stacked"])
@pytest.mark.parametrize("m", ALL_M)
def test_pcg_two_iterations_exact_in_every_tile_class(dev_ctx, m, stacked):
    """(A) n = 1, 2, 130 (two 64-row rounds and a ragged one) at every width of ALL_M, in the one-pass and the two-pass form
    (lfpsqp_ctx_set_onepass(-1) on a second context); m = 0, 1, 3, 1025 take the two-pass form in both."""
    ctx = dev_ctx
    c2 = twopass_ctx(ctx)
    worst = 0.0
    try:
        for n in (1, 2, 130):
            Z, D, r0, x0, one, two = case_A(1, n, m, stacked)
            assert two is not None or n < 2 or m < 1             # (only a one-dimensional solve or m = 0 may converge in one iteration)
            for c, name in ((ctx, "one-pass"), (c2, "two-pass")):
                worst = max(worst, check_A(Op(c, Z, D), r0, x0, one, two, f"n={n} m={m} {name}"))
    finally:
        c2.close()
    print(f"[pcg_exact A m={m} stacked={stacked}] x, r after two iterations: worst error / allowance {worst:.3f}")


@pytest.mark.parametrize("stacked", [False, True], ids=["plain", "stacked"])
@pytest.mark.parametrize("m", [5, 129, 513])
def test_pcg_two_iterations_exact_at_2049_rows(dev_ctx, m, stacked):
    """(A) n = 2049: 32 rounds of 64 rows and a ragged one of 1, several workgroups."""
    ctx = dev_ctx
    c2 = twopass_ctx(ctx)
    try:
        Z, D, r0, x0, one, two = case_A(2, 2049, m, stacked)
        assert two is not None
        w = [check_A(Op(c, Z, D), r0, x0, one, two, f"n=2049 m={m} {name}") for c, name in ((ctx, "one-pass"), (c2, "two-pass"))]
    finally:
        c2.close()
    print(f"[pcg_exact A n=2049 m={m} stacked={stacked}] worst error / allowance {max(w):.3f}")


@pytest.mark.parametrize("stacked", [False, True], ids=["plain", "stacked"])
@pytest.mark.parametrize("n,m", [(130, 5), (130, 33), (130, 130), (2049, 5), (2049, 33), (2049, 130)])
def test_pcg_two_iterations_exact_with_the_sparse_twin(dev_ctx, n, m, stacked):
    """(A) lfpsqp_basis.S set to the same entries (at most 8 per row): the two sparse products per iteration (P1SparseF, spmv_t, P2SparseF)."""
    Z, D, r0, x0, one, two = case_A(3, n, m, stacked, kmax=8)
    assert two is not None
    op = Op(dev_ctx, Z, D, sparse=True)
    assert 1 <= op.S.ell_width <= 8
    w = check_A(op, r0, x0, one, two, f"sparse n={n} m={m}")
    print(f"[pcg_exact A sparse n={n} m={m} stacked={stacked}] worst error / allowance {w:.3f}")


@pytest.mark.parametrize("stacked", [False, True], ids=["plain", "stacked"])
@pytest.mark.parametrize("m", [40, 100, 130, 300])
def test_pcg_two_iterations_exact_with_staged_stores(dev_ctx, monkeypatch, m, stacked):
    """(A) n = 4001: z (stacked: its two halves, kStageStreams = 2) waits in LDS and is stored in bursts; with the rounds per burst capped at
    1 (LFPSQP_STAGE_ROUNDS, read when a context is created) a workgroup goes through many bursts and a ragged last one.  Both == the
    reference."""
    Z, D, r0, x0, one, two = case_A(4, 4001, m, stacked)
    assert two is not None
    w = []
    for cap in ("", "1"):
        if cap:
            monkeypatch.setenv("LFPSQP_STAGE_ROUNDS", cap)
        else:
            monkeypatch.delenv("LFPSQP_STAGE_ROUNDS", raising=False)
        ctx = L.Context(0, dev_ctx.L)
        try:
            w.append(check_A(Op(ctx, Z, D), r0, x0, one, two, f"staged n=4001 m={m} cap={cap or 'unset'}"))
        finally:
            ctx.close()
    monkeypatch.delenv("LFPSQP_STAGE_ROUNDS", raising=False)
    print(f"[pcg_exact A staged m={m} stacked={stacked}] worst error / allowance {max(w):.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("stacked", [False, True], ids=["plain", "stacked"])
@pytest.mark.parametrize("m", [5, 128, 133, 260])
def test_pcg_two_iterations_exact_with_several_rounds_per_workgroup(gpu_lib, m, stacked):
    """(A, GPU only) n = 70001 = 1093 rounds of 64 rows and one of 49: a workgroup of the fused kernel turns its round loop several times, the
    last round ragged (as test_c_with_several_rounds_per_workgroup).  Thinned data (density 0.25 and below)."""
    ctx = L.Context(0, gpu_lib)
    try:
        assert not is_emu(ctx)
        Z, D, r0, x0, one, two = case_A(5, 70001, m, stacked, densities=(0.25, 0.1, 0.05))
        assert two is not None
        w = check_A(Op(ctx, Z, D), r0, x0, one, two, f"n=70001 m={m}")
    finally:
        ctx.close()
    print(f"[pcg_exact A n=70001 m={m} stacked={stacked}] worst error / allowance {w:.3f}")


# ================================================================================================================================
# (B) lfpsqp_pcg_pre: the first iteration exact
# ================================================================================================================================
MU_B = 4


def floor_log2(v):
    return int(v).bit_length() - 1


def pre_first_iteration(Z, ab, I, Ka, r0):
    """One iteration of src/retractions.jl:207-238 with M^-1 = D0^-1 - D0^-1 E Ka E' D0^-1, E = [Z; 0], mu = 4, x0 = 0, in integers.
    ab = (a, b): the diagonal block of the stacked operator A_f = mu I + [a; b][a b] + E E' (None: plain); I = (i11, i12, i22): the rows
    of D0^-1 (plain: 1 / mu).  Ka is the matrix APPLIED to sP = Z'(D0^-1 r)_x.  Unit of z, p: 2^-e."""
    Z = np.ascontiguousarray(Z, dtype=np.int64)
    Zt = np.ascontiguousarray(Z.T)
    N, m = Z.shape
    r0 = obj(r0)
    rx = r0[:N]
    if ab is None:
        e = 4                                                    # u = r / 4 (e = 2), z = u - v / 4 (e = 4)
        ux, uy = rx, None                                        # e = 2
    else:
        e = 0
        a, b = obj(ab[0]), obj(ab[1])
        i11, i12, i22 = (obj(v) for v in I)
        ry = r0[N:]
        ux, uy = i11 * rx + i12 * ry, i12 * rx + i22 * ry
    sP, sa = imul(Zt, ux)
    need(fits(sa))
    c1, ca = imul(np.ascontiguousarray(Ka, dtype=np.int64), sP)
    need(fits(ca))
    v, va = imul(Z, c1)
    need(fits(va))
    if ab is None:
        z = ux * 4 - v                                           # e = 4
        need(fits(abs(ux) * 4 + va))
        zx = z
    else:
        zx, zy = ux - i11 * v, uy - i12 * v
        need(fits(abs(ux) + abs(i11) * va) and fits(abs(uy) + abs(i12) * va))
        z = np.concatenate([zx, zy])
    rho = int(np.dot(z, r0))                                     # e
    need(int(np.dot(abs(z), abs(r0))) < 2 ** 53)
    tp, ta = imul(Zt, zx)                                        # J z = J p (beta * 0)
    need(fits(ta))
    ee, ea = imul(Z, tp)
    if ab is None:
        q = MU_B * z + ee
        need(fits(MU_B * abs(z) + ea))
    else:
        ww = a * zx + b * zy
        q = np.concatenate([MU_B * zx + a * ww + ee, MU_B * zy + b * ww])
        need(fits(abs(a * zx) + abs(b * zy)))
        need(fits(MU_B * abs(zx) + abs(a) * (abs(a * zx) + abs(b * zy)) + ea) and fits(MU_B * abs(zy) + abs(b) * (abs(a * zx) + abs(b * zy))))
    pq = int(np.dot(z, q))                                       # 2 e
    need(int(np.dot(abs(z), abs(q))) < 2 ** 53)
    need(pq != 0 and rho != 0)
    zd, qd = dbl(z, e), dbl(q, e)
    alpha = math.ldexp(float(rho) / float(pq), e)               # fl(rho / p'q): both exact, one correctly rounded quotient
    ref = {"z": zd, "p": zd, "q": qd, "x": alpha * zd, "alpha": alpha}           # x = fl(alpha p): one rounding per entry
    # r0 - alpha q as integers * 2^er, and the exponent of 1 ulp(max(|r0|, |alpha q|)) per entry
    A, ae = exact_ints(np.array([alpha]))
    A = int(A[0])
    er = ae - e
    if er <= 0:
        ref["r_int"], ref["r_e"] = r0 * 2 ** (-er) - A * q, er
    else:
        ref["r_int"], ref["r_e"] = r0 - A * q * 2 ** er, 0
    g = []
    for rv, qv in zip(r0.tolist(), q.tolist()):
        big = [floor_log2(abs(rv))] if rv else []
        if qv and A:
            big.append(floor_log2(abs(A * qv)) + ae - e)
        g.append(max(big) - 52 if big else None)
    ref["ulp_e"] = g
    return ref


def r_within_one_ulp(dev, ref):
    X, e = exact_ints(dev)
    c = min(e, ref["r_e"])
    diff = abs(X * 2 ** (e - c) - ref["r_int"] * 2 ** (ref["r_e"] - c))
    for d, g in zip(diff.tolist(), ref["ulp_e"]):
        if g is None:
            assert d == 0
        else:
            assert d * 2 ** max(c - g, 0) <= 2 ** max(g - c, 0), (d, c, g)


def case_B(seed, n, m, stacked, densities=(1.0, 0.25, 0.1, 0.05), symmetric=True):
    for density in densities:
        rng = np.random.default_rng([seed, n, m, int(stacked), int(density * 100)])
        Z = tern(rng, (n, m), density)
        K = tern(rng, (m, m), density)
        K = np.triu(K) + np.triu(K, 1).T if symmetric else K
        total = 2 * n if stacked else n
        r0 = rng.integers(-2, 3, total)
        r0[rng.integers(0, n)] = 1                               # (the x half is not all zero)
        ab = I = None
        if stacked:
            ab = [rng.integers(-1, 2, n), rng.integers(-1, 2, n)]
            I = [rng.integers(1, 3, n), rng.integers(-1, 2, n), rng.integers(1, 3, n)]
        try:
            ref = pre_first_iteration(Z, ab, I, K.T, r0)
        except NotExact:
            continue
        return Z, K, ab, I, r0, ref
    raise AssertionError("no exactly representable case found")


def op_B(ctx, Z, ab, sxy=None, sparse=False):
    n = Z.shape[0]
    D = None if ab is None else [ab[0], ab[1]] + (list(sxy) if sxy is not None else [np.ones(n), np.zeros(n)])
    return Op(ctx, Z, D, sparse=sparse)


def check_B(op, K, I, r0, ref, tag=""):
    rc, flag, it, o = op.solve(MU_B, np.zeros(len(r0)), r0, 0.0, 1, pre=(K,) + (tuple(I) if I is not None else (None, None, None)))
    assert (rc, flag, it) == (0, 1, 1), (tag, rc, flag, it)
    for k in ("z", "p", "q", "x"):
        np.testing.assert_array_equal(o[k], ref[k], err_msg=f"{tag}: {k}")
    r_within_one_ulp(o["r"], ref)


@pytest.mark.parametrize("stacked", [False, True], ids=["plain", "stacked"])
@pytest.mark.parametrize("m", ONEPASS_M)
def test_pcg_pre_first_iteration_exact_in_every_tile_class(dev_ctx, m, stacked):
    """(B) n = 1, 2, 130 at every one-pass width: PrecS0V<ST> (gemv_t), prec_small_kernel, PrecZE<ST>, PrecQE<ST>, PrecP3F."""
    for n in (1, 2, 130):
        Z, K, ab, I, r0, ref = case_B(11, n, m, stacked)
        check_B(op_B(dev_ctx, Z, ab), K, I, r0, ref, f"n={n} m={m}")


@pytest.mark.parametrize("stacked", [False, True], ids=["plain", "stacked"])
@pytest.mark.parametrize("n,m", [(2049, 33), (2049, 133), (4097, 33), (4097, 133)])
def test_pcg_pre_first_iteration_exact_over_several_workgroups(dev_ctx, n, m, stacked):
    Z, K, ab, I, r0, ref = case_B(12, n, m, stacked)
    check_B(op_B(dev_ctx, Z, ab), K, I, r0, ref, f"n={n} m={m}")


@pytest.mark.gpu
@pytest.mark.parametrize("stacked", [False, True], ids=["plain", "stacked"])
@pytest.mark.parametrize("m", [128, 260])
def test_pcg_pre_first_iteration_exact_with_several_rounds_per_workgroup(gpu_lib, m, stacked):
    """(B, GPU only) n = 70001, thinned data."""
    ctx = L.Context(0, gpu_lib)
    try:
        assert not is_emu(ctx)
        Z, K, ab, I, r0, ref = case_B(13, 70001, m, stacked, densities=(0.25, 0.1, 0.05))
        check_B(op_B(ctx, Z, ab), K, I, r0, ref, f"n=70001 m={m}")
    finally:
        ctx.close()


@pytest.mark.parametrize("stacked", [False, True], ids=["plain", "stacked"])
def test_pcg_pre_reads_k_by_columns(dev_ctx, stacked):
    """(B) A NON-symmetric K at m = 70 (two turns of the loop over 64 row groups in prec_small_kernel, the second with 6 rows).  The header
    calls K symmetric, column-major.  prec_small_kernel forms entry j of c1 = K sP from the m numbers stored at K + j * m, which is COLUMN j
    of the caller's matrix: it applies K' -- for a symmetric K the same thing.  So the call with K == the reference that applies K', the
    call with K' == the reference that applies K, and on this data the two differ."""
    n, m = 130, 70
    Z, K, ab, I, r0, ref_t = case_B(14, n, m, stacked, symmetric=False)
    assert (K != K.T).any()
    ref = pre_first_iteration(Z, ab, I, K, r0)
    assert (ref["z"] != ref_t["z"]).any()
    op = op_B(dev_ctx, Z, ab)
    check_B(op, K, I, r0, ref_t, "K")
    check_B(op, K.T, I, r0, ref, "K'")


def test_pcg_pre_ignores_the_row_scalings_of_a_stacked_basis(dev_ctx):
    """(B) lfpsqp_pcg_pre states its operator for E = [Jct; 0], the stacked basis with sx = 1, sy = 0.  OUTCOME RECORDED: with other
    integers in sx and sy the call gives, bit for bit, the E = [Jct; 0] answer -- it reads Dx and Dy and never sx, sy (they must only be
    non-NULL).  include/lfpsqp_hip.h says so next to lfpsqp_pcg_pre."""
    n, m = 130, 33
    Z, K, ab, I, r0, ref = case_B(15, n, m, True)
    rng = np.random.default_rng(15)
    for sxy in ([rng.integers(-2, 3, n), rng.integers(-2, 3, n)], [np.zeros(n), np.ones(n)], [np.full(n, np.nan), np.full(n, np.nan)]):
        check_B(op_B(dev_ctx, Z, ab, sxy=sxy), K, I, r0, ref, "sx, sy")


@pytest.mark.parametrize("stacked", [False, True], ids=["plain", "stacked"])
def test_pcg_pre_refusals_leave_the_vectors_alone(dev_ctx, stacked):
    """(B) m = 3 and m = 1025 and a sparse twin: LFPSQP_ERR_UNSUPPORTED; mu <= 0: LFPSQP_ERR_ARG; x, r, p, z (and q) as they were."""
    ctx = dev_ctx
    n = 130
    rng = np.random.default_rng(16)

    def refused(m, mu, sparse, want):
        Z = capped_rows(rng, tern(rng, (n, m), 1.0), 8)
        ab = [rng.integers(-1, 2, n), rng.integers(-1, 2, n)] if stacked else None
        I = [np.ones(n), np.zeros(n), np.ones(n)] if stacked else None
        op = op_B(ctx, Z, ab, sparse=sparse)
        total = 2 * n if stacked else n
        x0, r0 = rng.integers(-2, 3, total), rng.integers(-2, 3, total)
        rc, flag, it, o = op.solve(mu, x0, r0, 0.0, 3, pre=(np.eye(m),) + (tuple(I) if I is not None else (None, None, None)))
        assert rc == want, (m, mu, sparse, rc)
        mark = op.pack(np.full(total, MARK))
        np.testing.assert_array_equal(o["x"], op.pack(x0))
        np.testing.assert_array_equal(o["r"], op.pack(r0))
        np.testing.assert_array_equal(o["p"], np.full(op.nv, MARK))
        np.testing.assert_array_equal(o["z"], mark)
        np.testing.assert_array_equal(o["q"], mark)

    refused(3, 4.0, False, ERR_UNSUPPORTED)
    refused(1025, 4.0, False, ERR_UNSUPPORTED)
    refused(33, 4.0, True, ERR_UNSUPPORTED)
    refused(33, 0.0, False, ERR_ARG)
    refused(33, -1.0, False, ERR_ARG)
    refused(33, float("nan"), False, ERR_ARG)


# ================================================================================================================================
# (C) several iterations against the same statements in mpmath
# ================================================================================================================================
PREC = 280                                       # bits, set only inside mp_pcg and mp_rel (mpmath.workprec): no global setting
mpf = mpmath.mpf


def mpv(a):
    """binary64 numbers as mpf (exact at any working precision)."""
    return [mpf(float(v)) for v in np.asarray(a, dtype=np.float64).ravel().tolist()]


class MpOp:
    """J and J' of Op on lists of mpf (every sum by mpmath.fdot: accumulated exactly, rounded once to 280 bits)."""

    def __init__(self, Z, D=None):
        self.N, self.m = Z.shape
        Zo = np.array(mpv(Z), dtype=object).reshape(Z.shape)
        self.cols = [Zo[:, j].tolist() for j in range(self.m)]
        self.rows = [Zo[i, :].tolist() for i in range(self.N)]
        self.D = [mpv(d) for d in D] if D is not None else None

    def A(self, p, mu):
        """(J'J + mu I) p"""
        N = self.N
        if self.D is None:
            t = [mpmath.fdot(c, p) for c in self.cols]
            return [mpmath.fdot(row, t) + mu * pi for row, pi in zip(self.rows, p)]
        Dx, Dy, sx, sy = self.D
        px, py = p[:N], p[N:]
        w = [Dx[i] * px[i] + Dy[i] * py[i] for i in range(N)]
        v = [sx[i] * px[i] + sy[i] * py[i] for i in range(N)]
        t = [mpmath.fdot(c, v) for c in self.cols]
        a = [mpmath.fdot(row, t) for row in self.rows]
        return [Dx[i] * w[i] + sx[i] * a[i] + mu * px[i] for i in range(N)] + [Dy[i] * w[i] + sy[i] * a[i] + mu * py[i] for i in range(N)]

    def M(self, r, K, I, mu):
        """z = D0^-1 r - D0^-1 E K E' D0^-1 r, E = [Z; 0]; I = rows of D0^-1 (None: 1 / mu); K as the caller's doubles."""
        N = self.N
        if I is None:
            i11 = [mpf(1) / mu] * N
            ux, uy = [i11[i] * r[i] for i in range(N)], None
        else:
            i11, i12, i22 = I
            ux = [i11[i] * r[i] + i12[i] * r[N + i] for i in range(N)]
            uy = [i12[i] * r[i] + i22[i] * r[N + i] for i in range(N)]
        sP = [mpmath.fdot(c, ux) for c in self.cols]
        c1 = [mpmath.fdot(krow, sP) for krow in K]
        v = [mpmath.fdot(row, c1) for row in self.rows]
        zx = [ux[i] - i11[i] * v[i] for i in range(N)]
        return zx if I is None else zx + [uy[i] - i12[i] * v[i] for i in range(N)]


@mpmath.workprec(PREC)
def mp_pcg(op, mu, b, iters, pre=None):
    """The statements of pcg! (src/retractions.jl:202-238) with x0 = 0 -> [(x_k, r_k) for k = 1 .. iters]."""
    mu = mpf(mu)
    r = mpv(b)
    x = [mpf(0)] * len(r)
    p = [mpf(0)] * len(r)
    rho = mpf(1)
    if pre is not None:
        K = [mpv(row) for row in np.asarray(pre[0])]
        I = [mpv(a) for a in pre[1:]] if pre[1] is not None else None
    out = []
    for _ in range(iters):
        z = r if pre is None else op.M(r, K, I, mu)              # :209
        rho_prev, rho = rho, mpmath.fdot(z, r)                   # :213
        beta = rho / rho_prev                                    # :216
        p = [zi + beta * pi for zi, pi in zip(z, p)]             # :217
        q = op.A(p, mu)                                          # :220-222
        alpha = rho / mpmath.fdot(p, q)                          # :227
        x = [xi + alpha * pi for xi, pi in zip(x, p)]            # :232
        r = [ri - alpha * qi for ri, qi in zip(r, q)]            # :233
        out.append((x, r))
    return out


@mpmath.workprec(PREC)
def mp_rel(got, ref, scale=None):
    """|got - ref|_2 / |scale|_2 (scale = ref unless given)."""
    num = mpmath.sqrt(mpmath.fsum((mpf(float(g)) - v) ** 2 for g, v in zip(got.tolist(), ref)))
    den = mpmath.sqrt(mpmath.fsum(v * v for v in (ref if scale is None else scale)))
    return float(num / den)


def dense_J(Z, D):
    """J as a dense matrix for the float64 oracle: (N + m) x 2N stacked, m x N plain."""
    if D is None:
        return np.ascontiguousarray(Z.T)
    Dx, Dy, sx, sy = D
    return np.block([[np.diag(Dx), np.diag(Dy)], [Z.T * sx[None, :], Z.T * sy[None, :]]])


def d0_inverse(a, b, mu):
    det = mu * (a * a + b * b + mu)
    return (b * b + mu) / det, -(a * b) / det, (a * a + mu) / det


def oracle_M(Z, K, I, mu):
    N = Z.shape[0]

    def M_(z, r):
        if I is None:
            ux = r / mu
            z[:] = ux - (Z @ (K @ (Z.T @ ux))) / mu
        else:
            ux, uy = I[0] * r[:N] + I[1] * r[N:], I[1] * r[:N] + I[2] * r[N:]
            v = Z @ (K @ (Z.T @ ux))
            z[:N] = ux - I[0] * v
            z[N:] = uy - I[1] * v
        return z
    return M_


def oracle_pcg(Z, D, mu, b, tol, maxiter, pre=None):
    J = dense_J(Z, D)
    x, r = np.zeros(len(b)), np.array(b, dtype=np.float64)
    M_ = (lambda z, r_: np.copyto(z, r_)) if pre is None else oracle_M(Z, pre[0], pre[1:] if pre[1] is not None else None, mu)
    p = np.zeros(len(b))
    flag, it = R.pcg_(mu, J, M_, x, r, p, np.zeros(len(b)), np.zeros(J.shape[0]), tol, maxiter)
    return flag, it, x, r, p


def real_case(seed, n, m, form, mu):
    """Gaussian Jct / sqrt(n); stacked: random unit (Dx, Dy) and general sx, sy (pre: sx = 1, sy = 0, the operator lfpsqp_pcg_pre is stated
    for).  -> Z, D, b, kappa = (sigma_1^2 + mu) / mu of the operator."""
    rng = np.random.default_rng([seed, n, m])
    Z = np.asfortranarray(rng.standard_normal((n, m)) / math.sqrt(n))
    D = None
    if "stacked" in form:
        th = rng.uniform(0, 2 * math.pi, n)
        sxy = [np.ones(n), np.zeros(n)] if "pre" in form else [rng.uniform(-0.7, 0.7, n), rng.uniform(-0.7, 0.7, n)]
        D = [np.cos(th), np.sin(th)] + sxy
    b = rng.standard_normal(2 * n if D is not None else n)
    s1 = np.linalg.norm(dense_J(Z, D), 2)
    return Z, D, b, (s1 * s1 + mu) / mu, s1 * s1 + mu


def check_C(ctx, Z, D, b, mu, kappa, tag, pre=None, sparse=False, Ks=(1, 2, 4), op_ctx=None):
    """Device and float64 oracle after K iterations against the mpmath trajectory: |x_K - x_ref| <= K kappa gamma_{n+m+4} |x_ref| and
    |r_K - r_ref| <= the same * |b|, n the length of the solve's vectors (2N stacked: its dot products have 2N terms); the oracle must
    stay below a quarter of it.  -> worst (device, oracle) error / bound."""
    assert kappa <= 16.0, kappa
    nv, m = len(b), Z.shape[1]
    traj = mp_pcg(MpOp(Z, D), mu, b, max(Ks), pre)
    op = Op(ctx, Z, D, sparse=sparse)
    bmp = mpv(b)
    worst = [0.0, 0.0]
    for K in Ks:
        bound = K * kappa * float(gamma(nv + m + 4))
        xr, rr = traj[K - 1]
        rc, flag, it, o = op.solve(mu, np.zeros(nv), b, 0.0, K, pre=pre)
        assert (rc, flag, it) == (0, 1, K), (tag, rc, flag, it)
        f0, i0, x0, r0, _ = oracle_pcg(Z, D, mu, b, 0.0, K, pre)
        assert (f0, i0) == (1, K)
        e_dev = max(mp_rel(o["x"], xr), mp_rel(o["r"], rr, bmp)) / bound
        e_ora = max(mp_rel(x0, xr), mp_rel(r0, rr, bmp)) / bound
        print(f"[pcg_exact C {tag} K={K}] kappa {kappa:.2f}: error / bound: oracle {e_ora:.2e}, device {e_dev:.2e}")
        assert e_ora <= 0.25, (tag, K, e_ora)
        assert e_dev <= 1.0, (tag, K, e_dev)
        worst = [max(worst[0], e_dev), max(worst[1], e_ora)]
    return worst


C_SHAPES = [(513, 5, 0.125), (1025, 37, 0.25), (700, 130, 0.25), (300, 261, 0.5)]


@pytest.mark.parametrize("form", ["plain", "stacked"])
@pytest.mark.parametrize("n,m,mu", C_SHAPES)
def test_pcg_trajectory_against_mpmath(dev_ctx, n, m, mu, form):
    Z, D, b, kappa, _ = real_case(21, n, m, form, mu)
    check_C(dev_ctx, Z, D, b, mu, kappa, f"{form} ({n}, {m})")


def test_pcg_trajectory_against_mpmath_with_the_sparse_twin(dev_ctx):
    n, m, mu = 1025, 37, 0.25
    Z, D, b, kappa, _ = real_case(22, n, m, "plain", mu)
    check_C(dev_ctx, Z, D, b, mu, kappa, f"sparse ({n}, {m})", sparse=True)


def pre_for(Z, D, mu, weight):
    """(K, i11, i12, i22) with the true D0^-1 and K = (I + weight E'D0^-1 E)^-1 (weight = 1: the exact preconditioner), symmetrised."""
    n, m = Z.shape
    I = d0_inverse(D[0], D[1], mu) if D is not None else None
    i11 = I[0] if I is not None else np.full(n, 1.0 / mu)
    K = np.linalg.inv(np.eye(m) + weight * (Z.T @ (i11[:, None] * Z)))
    K = 0.5 * (K + K.T)
    return (K,) + (tuple(I) if I is not None else (None, None, None))


@pytest.mark.parametrize("form", ["pre", "pre-stacked"])
@pytest.mark.parametrize("n,m,mu", [(1025, 37, 0.25), (700, 130, 0.25)])
def test_pcg_pre_trajectory_against_mpmath(dev_ctx, n, m, mu, form):
    """lfpsqp_pcg_pre with the true D0^-1 and the INEXACT K = (I + 0.3 E'D0^-1 E)^-1: several meaningful iterations."""
    Z, D, b, kappa, _ = real_case(23, n, m, form, mu)
    check_C(dev_ctx, Z, D, b, mu, kappa, f"{form} ({n}, {m}) inexact K", pre=pre_for(Z, D, mu, 0.3))


@pytest.mark.parametrize("form", ["pre", "pre-stacked"])
@pytest.mark.parametrize("n,m,mu", [(1025, 37, 0.25), (700, 130, 0.25)])
def test_pcg_pre_with_the_exact_k_converges_in_one_iteration(dev_ctx, n, m, mu, form):
    """The exact K = (I + E'D0^-1 E)^-1 and one iteration: inside the bound of the trajectory, and additionally
    |r_1| <= kappa gamma_{n+m+4} |A_f|, |A_f| = sigma_1^2 + mu."""
    Z, D, b, kappa, normA = real_case(23, n, m, form, mu)
    pre = pre_for(Z, D, mu, 1.0)
    check_C(dev_ctx, Z, D, b, mu, kappa, f"{form} ({n}, {m}) exact K", pre=pre, Ks=(1,))
    rc, flag, it, o = Op(dev_ctx, Z, D).solve(mu, np.zeros(len(b)), b, 0.0, 1, pre=pre)
    bound = kappa * float(gamma(len(b) + m + 4))
    r1, lim = np.linalg.norm(o["r"]), bound * normA
    print(f"[pcg_exact C {form} ({n}, {m}) exact K] |r| {np.linalg.norm(b):.1e} -> {r1:.1e} (limit {lim:.1e})")
    assert r1 <= lim


BIG = 2.0 ** 20


@pytest.mark.parametrize("m", [130, 261])
@pytest.mark.parametrize("spot", ["last row", "row 63", "row 64", "row 15", "row 16", "last column"])
def test_pcg_trajectory_with_a_single_large_entry(dev_ctx, m, spot):
    """One entry of 2^20 in Jct (the pattern of test_gram_single_large_entry) at the edges of the 64-row and 16-row rounds and in the last
    column.  mu = 2^37 keeps kappa = (sigma_1^2 + mu) / mu near 9: the entry carries (2^40 + mu) / mu of its row of the operator, so a row
    or column dropped from either product moves x by about 1 / sqrt(n) of its norm -- nine orders above the bound."""
    n, mu = 300, 2.0 ** 37
    Z, D, b, _, _ = real_case(24, n, m, "plain", mu)
    i, j = {"last row": (n - 1, m // 2), "last column": (100, m - 1)}.get(spot) or (int(spot.split()[1]), m // 2)
    Z[i, j] = BIG
    s1 = np.linalg.norm(Z, 2)
    check_C(dev_ctx, Z, D, b, mu, (s1 * s1 + mu) / mu, f"2^20 at {spot} m={m}")


# ================================================================================================================================
# (D) stopping and the launches queued ahead of the device-side stop
# ================================================================================================================================
D_N, D_M, D_MU = 1500, 40, 0.05


def case_D(form):
    rng = np.random.default_rng(31)
    Z = np.asfortranarray(rng.standard_normal((D_N, D_M)) / math.sqrt(D_N))
    D = pre = None
    if form == "stacked":
        th = rng.uniform(0, 2 * math.pi, D_N)
        D = [0.2 * np.cos(th), 0.2 * np.sin(th), rng.uniform(-0.2, 0.2, D_N), rng.uniform(-0.2, 0.2, D_N)]   # (well conditioned: |r_k| falls)
    if form == "pre":
        pre = pre_for(Z, None, D_MU, 0.3)
    b = rng.standard_normal(2 * D_N if D is not None else D_N)
    return Z, D, pre, b


def op_D(ctx, form, Z, D):
    return Op(ctx, Z, D, sparse=(form == "sparse"))


@pytest.mark.parametrize("form", ["one-pass", "two-pass", "sparse", "stacked", "pre"])
def test_stop_by_tol_leaves_the_bits_of_stop_by_maxiter(dev_ctx, form):
    """The host queues iterations ahead of the device-side stop (the status is read two iterations late): every kernel of an iteration
    queued after the stop has to skip.  For k = 1, 2, 3, 5 a solve with tol between |r_{k-1}| and |r_k| and maxiter = 50 returns iters = k,
    flag = 0 and, bit for bit, the x, r, p, z (lfpsqp_pcg_pre: and q) of the solve with tol = 0, maxiter = k (flag = 1)."""
    ctx = twopass_ctx(dev_ctx) if form == "two-pass" else dev_ctx
    try:
        Z, D, pre, b = case_D(form)
        op = op_D(ctx, form, Z, D)
        x0 = np.zeros(len(b))
        hist, runs = [float(np.linalg.norm(b))], {}
        for k in range(1, 6):
            rc, flag, it, o = op.solve(D_MU, x0, b, 0.0, k, pre=pre)
            assert (rc, flag, it) == (0, 1, k)
            runs[k] = o
            hist.append(float(np.linalg.norm(o["r"])))
        for k in (1, 2, 3, 5):
            # the loop tests |r_j| > tol from j = 1 on (norm_res starts at Inf; |r_1| may exceed |r_0|): it stops at k when |r_k| <= tol < |r_j|
            # for 1 <= j < k -- a tol well inside that gap, which the input must leave open
            above = min(hist[1:k], default=4.0 * hist[1])
            assert hist[k] < 0.9 * above, (k, hist)
            tol = math.sqrt(above * hist[k])
            rc, flag, it, o = op.solve(D_MU, x0, b, tol, 50, pre=pre)
            assert (rc, flag, it) == (0, 0, k), (form, k, rc, flag, it)
            for name in runs[k]:
                np.testing.assert_array_equal(o[name], runs[k][name], err_msg=f"{form} k={k}: {name}")
    finally:
        if form == "two-pass":
            ctx.close()


@pytest.mark.parametrize("form", ["one-pass", "two-pass", "sparse", "stacked", "pre"])
def test_maxiter_zero_and_negative(dev_ctx, form):
    """maxiter = 0: iters = 0, flag = 1 (the reference's i == maxiter); maxiter = -1: iters = 0, flag = 0.  x and r untouched, p zero-filled
    (src/retractions.jl:204)."""
    ctx = twopass_ctx(dev_ctx) if form == "two-pass" else dev_ctx
    try:
        Z, D, pre, b = case_D(form)
        op = op_D(ctx, form, Z, D)
        x0 = np.arange(len(b)) % 7 - 3.0
        for maxiter, want in ((0, 1), (-1, 0)):
            rc, flag, it, o = op.solve(D_MU, x0, b, 1e-9, maxiter, pre=pre)
            assert (rc, flag, it) == (0, want, 0)
            np.testing.assert_array_equal(o["x"], x0)
            np.testing.assert_array_equal(o["r"], b)
            assert not o["p"].any()
    finally:
        if form == "two-pass":
            ctx.close()


@pytest.mark.parametrize("form", ["one-pass", "two-pass", "sparse", "stacked", "pre"])
def test_nan_in_the_right_hand_side_stops_after_one_iteration(dev_ctx, form):
    """NaN > tol is false: iters = 1, flag = 0 with maxiter = 6, as the oracle (the host loop is bounded by maxiter: this cannot spin);
    p is NaN where the oracle's is."""
    ctx = twopass_ctx(dev_ctx) if form == "two-pass" else dev_ctx
    try:
        Z, D, pre, b = case_D(form)
        b[len(b) // 3] = np.nan
        f0, i0, _, _, p0 = oracle_pcg(Z, D, D_MU, b, 1e-9, 6, pre)
        assert (f0, i0) == (0, 1)
        rc, flag, it, o = op_D(ctx, form, Z, D).solve(D_MU, np.zeros(len(b)), b, 1e-9, 6, pre=pre, gap=False)    # (NaN * 0 in the gap)
        assert (rc, flag, it) == (0, 0, 1)
        # the first beta = rho / 1 is NaN (:216): p = z + NaN * 0 is NaN wherever the oracle's is
        np.testing.assert_array_equal(np.isnan(o["p"]), np.isnan(p0))
        assert np.isnan(p0).all() or pre is not None
    finally:
        if form == "two-pass":
            ctx.close()


@pytest.mark.parametrize("tol", [math.inf, math.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("form", ["one-pass", "two-pass", "sparse", "stacked", "pre"])
def test_tol_inf_and_nan_run_no_iteration(dev_ctx, form, tol):
    """norm_res = Inf; `while norm_res > tol` is false for tol = +Inf and for tol = NaN (src/retractions.jl:202,207): the reference runs no
    iteration, the oracle returns (flag, iters) = (0, 0); x and r stay as they were (PInit / PrecInit start the solve only when
    maxit > 0 && Inf > tol)."""
    ctx = twopass_ctx(dev_ctx) if form == "two-pass" else dev_ctx
    try:
        Z, D, pre, b = case_D(form)
        f0, i0, xo, ro, _ = oracle_pcg(Z, D, D_MU, b, tol, 5, pre)
        assert (f0, i0) == (0, 0) and not xo.any() and np.array_equal(ro, b)
        x0 = np.arange(len(b)) % 7 - 3.0
        rc, flag, it, o = op_D(ctx, form, Z, D).solve(D_MU, x0, b, tol, 5, pre=pre)
        assert (rc, flag, it) == (0, 0, 0), (form, tol, rc, flag, it)
        np.testing.assert_array_equal(o["x"], x0)
        np.testing.assert_array_equal(o["r"], b)
        assert not o["p"].any()
    finally:
        if form == "two-pass":
            ctx.close()


# ================================================================================================================================
# (E) the fused solve against the statement-by-statement loop on the device primitives
# ================================================================================================================================
@pytest.mark.parametrize("form", ["plain", "stacked"])
def test_fused_pcg_against_the_loop_on_the_primitives(dev_ctx, form):
    """projpenalty.pcg_ with a host callable as M! runs the reference's loop on lfpsqp_gemv_t / _n (lfpsqp_q_gemv_t / _n), dot, axpby,
    nrm2 -- kernels under exact tests of their own.  With M! = copy it has to take the iteration count of lfpsqp_pcg and give its x within
    the bound of (C), K the iteration count."""
    from types import SimpleNamespace
    from lfpsqp_jl_amd.inequality import StackedVector
    from lfpsqp_jl_amd.projpenalty import _JacPlain, _JacStacked, pcg_
    ctx = dev_ctx
    n, m, mu = 1025, 37, 0.25
    Z, D, b, kappa, _ = real_case(41, n, m, "pre-stacked" if form == "stacked" else "plain", mu)        # (_JacStacked: sx = 1, sy = 0)
    assert kappa <= 16.0
    Jct = ctx.matrix(n, m, Z)
    w = L.ProjPenaltyWork(ctx, m, n, form == "stacked")
    if form == "stacked":
        w.DxS.upload(D[0])
        w.DyS.upload(D[1])
        J = _JacStacked(SimpleNamespace(Jct=Jct), w)
        mk = lambda data=None: StackedVector(ctx, n).upload2(data) if data is not None else StackedVector(ctx, n)
        get = lambda v: v.download2()
    else:
        J = _JacPlain(Jct, w)
        mk = lambda data=None: ctx.vector(n, data)
        get = lambda v: v.download()

    def fused(tol, maxiter):
        x, r = mk(), mk(b)
        flag, it = pcg_(mu, J, L.no_precondition, x, r, w.p, w.z, None, tol, maxiter)
        return flag, it, get(x), get(r)

    k = 6
    _, i5, _, r5 = fused(0.0, k - 1)
    _, i6, _, r6 = fused(0.0, k)
    assert (i5, i6) == (k - 1, k) and np.linalg.norm(r6) < 0.9 * np.linalg.norm(r5)
    tol = math.sqrt(np.linalg.norm(r5) * np.linalg.norm(r6))
    flag, it, xf, rf = fused(tol, 50)
    x, r = mk(), mk(b)
    flag_s, it_s = pcg_(mu, J, (lambda z_, r_: z_.copy_from(r_)), x, r, w.p, w.z, None, tol, 50)
    xs = get(x)
    assert (flag, it) == (flag_s, it_s) == (0, k)
    bound = k * kappa * float(gamma(len(b) + m + 4))
    err = np.linalg.norm(xf - xs) / np.linalg.norm(xs)
    print(f"[pcg_exact E {form}] {it} iterations, |x_fused - x_loop| / |x_loop| = {err:.2e} = {err / bound:.2e} of the bound")
    assert err <= bound
