"""projcg! with a TRIDIAGONAL Hessian and BOUNDS on the one-pass iteration (lfpsqp_projcg_tridiag over a stacked basis).

With bounds the reference's Newton map is blockdiag(T + diag(2 lamy q), diag(2 lamy s)) (src/inequality_helper.jl:144-158) over the stacked
variables [x; y], and projcg! projects with Q = [[diag Dx; diag Dy], [sx.*Z; sy.*Z]] (src/optimize.jl:366-381).  The one-pass form splits the
products the pass cannot form row by row as include/lfpsqp_hip.h and the comment above PcgFuseTri state; checked here: those identities on the
host, the C entry alone against the oracle's projcg! with the augmented map as a matrix-free operator (four bound types, sizes at tile / pad
multiples and +-1, narrow to wide tiles, materialised and factored bases, couplings of both signs and a reduced operator that is not
diagonally dominant, multipliers, the iteration limit, negative curvature), the callback path with the same operator, ChainSeparableLinear
under box bounds and under ball + box bounds through `optimize` against the oracle, and the shapes that are still refused."""
import ctypes as C
import math

import numpy as np
import pytest

import lfpsqp_jl_amd as L
from lfpsqp_jl_amd import _capi
from oracle import lfpsqp_ref as R
from oracle import synth

from .test_bounds_only import _four_way
from .test_capi_retractions import _is_emu, _note, _sep_host


def _sxsy(Dx, Dy):
    return Dy * Dy, -Dx * Dy                                           # as lfpsqp_inequality_gradient builds them (ineq.hip)


def test_stacked_one_pass_identities_on_the_host():
    """The three identities of the comment above PcgFuseTri, in numpy on a random 37 x 5 case: M = Q_Z'A Q_Z = Z' At Z, the Z-block of
    Q'(A gp) from u and q, and gp'A gp = u'A u - 2 t'(Q_Z'A u) + t'M t."""
    rng = np.random.default_rng(5)
    n, m = 37, 5
    dx, dy = rng.standard_normal(n), rng.standard_normal(n)
    nrm = np.sqrt(dx * dx + dy * dy)
    Dx, Dy = dx / nrm, dy / nrm
    sx, sy = _sxsy(Dx, Dy)
    Z = rng.standard_normal((n, m))
    ax, ay, off = 2.0 + rng.random(n), rng.random(n), rng.standard_normal(n - 1)
    T = np.diag(ax) + np.diag(off, 1) + np.diag(off, -1)
    A = np.block([[T, np.zeros((n, n))], [np.zeros((n, n)), np.diag(ay)]])
    QZ = np.vstack([sx[:, None] * Z, sy[:, None] * Z])
    t = rng.standard_normal(m)
    rx, ry = rng.standard_normal(n), rng.standard_normal(n)
    ww = Dx * rx + Dy * ry
    ux, uy = rx - Dx * ww, ry - Dy * ww
    acc = Z @ t
    gp = np.concatenate([ux - sx * acc, uy - sy * acc])
    # M
    At = np.diag(sx * sx * ax + sy * sy * ay) + np.diag(sx[:-1] * off * sx[1:], 1) + np.diag(sx[:-1] * off * sx[1:], -1)
    M = QZ.T @ A @ QZ
    assert np.abs(M - Z.T @ At @ Z).max() <= 1e-13 * np.abs(M).max()
    # the Z-block of Q'(A gp)
    q = np.zeros(n)
    q[1:] += off * ux[:-1]
    q[:-1] += off * ux[1:]
    zb = Z.T @ (sx * (ax * ux + q) + sy * ay * uy) - M @ t
    ref = QZ.T @ (A @ gp)
    assert np.abs(zb - ref).max() <= 1e-13 * np.abs(ref).max()
    # gp'A gp
    u = np.concatenate([ux, uy])
    uAu = np.sum(ux * (ax * ux + q)) + np.sum(ay * uy * uy)
    assert abs(uAu - u @ A @ u) <= 1e-13 * abs(u @ A @ u)
    gAg = uAu - 2.0 * t @ (QZ.T @ (A @ u)) + t @ M @ t
    assert abs(gAg - gp @ A @ gp) <= 1e-13 * abs(gp @ A @ gp)


class _AugTriRef:
    """The augmented Newton map blockdiag(T, diag(ay)) on 2n-vectors, T = diag(ax) + couplings e (the oracle side)."""

    def __init__(self, ax, e, ay):
        self.ax, self.e, self.ay = ax, e, ay

    def _op(self, v):
        n = len(self.ax)
        out = np.empty(2 * n)
        out[:n] = self.ax * v[:n]
        out[:n - 1] += self.e * v[1:n]
        out[1:n] += self.e * v[:n - 1]
        out[n:] = self.ay * v[n:]
        return out

    def mul_(self, dest, v, al=None, be=None):
        t = self._op(v)
        dest[:] = t if al is None else al * t + be * dest
        return dest

    def adjoint(self):
        return self


def _stacked_problem(ctx, n, m, factored, view=False):
    """A stacked basis at a point with rows of all four bound types (device), and the oracle's Q over the SAME Z (so multipliers compare
    entry by entry)."""
    xl, xu = _four_way(n)
    xaug = np.zeros(2 * n)
    xaug[:n] = 0.9 * synth.hash_vector(2, n)
    idata0 = R.InequalityData(xl, xu)
    R.generate_initial_y_(xaug, idata0)
    xaug[n:] += 0.2 * synth.hash_vector(9, n)                          # off the bound manifold: (Dx, Dy) of every direction
    idata = L.InequalityData(ctx, xl, xu)
    X = L.StackedVector(ctx, n).upload2(xaug)
    Jh = np.asfortranarray(synth.hash_matrix(1, n, m))
    J = ctx.matrix(n, m, Jh)
    idc = L.InequalityDecomp(ctx, n, m, J, factored=factored)
    L.inequality_gradient_(idc, X, idata)
    Wg = np.zeros((m, m), order='F')
    idc.Sigma, idc.Vt, idc.rank = L.ksvd_(idc.Jct, idc.Z, w2=idc.sx, W=Wg)
    if factored:
        idc.W = Wg
        Zh = Jh @ Wg
    else:
        Zh = idc.Z.download()
        if view:
            idc.Z = idc.Z.view(ctx.vector(n, np.ones(n)))
    Dx, Dy, S = idc.Dx.download(), idc.Dy.download(), idc.S.download()
    sx, sy = _sxsy(Dx, Dy)
    rank = idc.rank
    idc0 = R.InequalityDecomp(np.asfortranarray(np.vstack([sx[:, None] * Zh, sy[:, None] * Zh])), idc.Sigma, idc.Vt, Dx, Dy, S, Jh, rank)
    return L.InequalityDecompProject(idc), R.InequalityDecompProject(idc0), (Dx, Dy, sx, sy), rank


def _operator(ctx, n, ax, e, ay):
    dg = L.StackedVector(ctx, n).upload2(np.concatenate([ax, ay]))
    return L.TridiagonalOperator(0.0, dg, ctx.vector(n, np.concatenate([e, [123.0]])))      # (the last coupling must be ignored)


def _solve_c(ctx, A, P, b, n, m, tol, maxit=None, want_lambda=True):
    """lfpsqp_projcg_tridiag itself (no fall-back): returns rc, iterations, nr, x, lambda."""
    x, lam = L.StackedVector(ctx, n), ctx.vector(n + m)
    work = L.ProjCGWork(ctx, 0, m, stacked_N=n)
    Av = L.StackedVector(ctx, n)
    it, nr = _capi.c_i64(), C.c_double()
    a_c, u_c, w_c = A._c(), P._c(), work._c()
    rc = ctx.L.lfpsqp_projcg_tridiag(ctx.h, x.h, lam.h, C.byref(a_c), Av.h, C.byref(u_c), b.h, None, float(tol),
                                     int(2 * n + m if maxit is None else maxit), 2 * n, 1 if want_lambda else 0, C.byref(w_c), C.byref(it), C.byref(nr))
    return rc, it.value, nr.value, x, lam


# (n, m, factored, dominant): n at the tile / padding granularity (2048) and +-1, m from the narrowest one-pass tile to past a tile width
_CASES = [(2047, 4, False, True), (2048, 16, True, False), (2049, 128, False, False), (4096, 130, True, True), (1500, 16, False, True)]


@pytest.mark.parametrize("n,m,factored,dominant", _CASES)
def test_stacked_tridiagonal_solver_follows_the_oracle(dev_ctx, n, m, factored, dominant):
    ctx = dev_ctx
    P, P0, (Dx, Dy, sx, sy), rank = _stacked_problem(ctx, n, m, factored)
    assert rank == m
    ax = 4.0 * synth.hash_vector(3, n) + 5.0
    e = (0.8 if dominant else 3.0) * synth.hash_vector(15, n - 1)     # both signs
    ay = 0.5 + synth.hash_vector(16, n) ** 2
    if not dominant:
        from scipy.linalg import eigvalsh_tridiagonal
        ax = ax + 4.5                                                  # T stays positive definite (checked) ...
        assert eigvalsh_tridiagonal(ax, e, select='i', select_range=(0, 0))[0] > 0.05
        # ... but the reduced operator's tridiagonal At is not diagonally dominant: the Gram pass with the negative weights runs
        ad, ao = sx * sx * ax + sy * sy * ay, sx[:-1] * e * sx[1:]
        cw = ad - np.abs(np.concatenate([ao, [0.0]])) - np.abs(np.concatenate([[0.0], ao]))
        assert np.any(cw < 0)
    A = _operator(ctx, n, ax, e, ay)
    Aref = _AugTriRef(ax, e, ay)
    bh = synth.hash_vector(4, 2 * n)
    tmp = np.zeros(n + m)
    R.mul_(tmp, R.adj(P0), bh)
    R.mul_(bh, P0, tmp, -1.0, 1.0)                                      # a right-hand side in the tangent space, like optimize's d
    b = L.StackedVector(ctx, n).upload2(bh)
    for tol, maxit in ((1e-10, None), (1e-300, 5)):
        x0, l0 = np.zeros(2 * n), np.zeros(n + m)
        i0, nr0 = R.projcg_(x0, l0, Aref, P0, bh, np.zeros(n + m), tol=tol, maxit=maxit)
        rc, i1, nr1, x, lam = _solve_c(ctx, A, P, b, n, m, tol, maxit)
        assert rc == 0, ctx.L.lfpsqp_last_error(ctx.h) if hasattr(ctx.L, "lfpsqp_last_error") else rc
        xd, ld = x.download2(), lam.download()
        dx_ = np.linalg.norm(xd - x0) / np.linalg.norm(x0)
        dl_ = np.abs(ld - l0).max() / np.abs(l0).max()
        print(f"[stacked tridiag] n={n} m={m} factored={factored} dominant={dominant} maxit={maxit}: iterations {i1} (oracle {i0}), "
              f"x {dx_:.1e}, lambda {dl_:.1e}, nr {nr1:.3e} / {nr0:.3e}")
        assert i1 == i0 and (maxit is not None or i1 > 3)
        assert nr1 == pytest.approx(nr0, rel=1e-6)
        assert dx_ <= 1e-10
        assert dl_ <= 1e-9                                             # lambda = Q'(b - A x): an n-sized product of x, one digit more
        if factored:
            continue                                                   # (the callback path needs a materialised basis)
        # the callback path (lfpsqp_projcg_op, two passes per iteration) with the same operator: equal counts, the same iterate
        A.fused = False
        x2, lam2 = L.StackedVector(ctx, n), ctx.vector(n + m)
        i2, nr2 = L.projcg_(x2, lam2, A, P, b, None, tol=tol, maxit=maxit, work=L.ProjCGWork(ctx, 0, m, stacked_N=n))
        A.fused = True
        d2_ = np.linalg.norm(x2.download2() - xd) / np.linalg.norm(x0)
        print(f"[stacked tridiag] ... against the callback path: iterations {i2}, x {d2_:.1e}")
        assert i2 == i1 and d2_ <= 1e-10
    # negative curvature (src/projcg.jl:77-82): the exit, the normalised direction, NaN multipliers
    x0, l0 = np.zeros(2 * n), np.zeros(n + m)
    i0, nr0 = R.projcg_(x0, l0, _AugTriRef(-ax, e, ay), P0, bh, np.zeros(n + m), tol=1e-10)
    rc, i1, nr1, x, lam = _solve_c(ctx, _operator(ctx, n, -ax, e, ay), P, b, n, m, 1e-10)
    assert rc == 0 and (i1, nr1) == (i0, nr0) and math.isinf(nr1)
    assert np.linalg.norm(x.download2() - x0) <= 1e-10 and np.all(np.isnan(lam.download()))


def test_stacked_tridiagonal_product(dev_ctx):
    """lfpsqp_tridiag_mul over a stacked pair: the couplings on the x half, the y half diagonal, the gap left at zero."""
    ctx = dev_ctx
    for n in (1, 2, 3, 2047, 2048, 2049):
        ax, ay = 4.0 * synth.hash_vector(3, n) + 5.0, synth.hash_vector(16, n)
        e = 0.8 * synth.hash_vector(15, max(n - 1, 1))[:n - 1]
        vh = synth.hash_vector(7, 2 * n)
        A = _operator(ctx, n, ax, e, ay)
        out = L.StackedVector(ctx, n)
        A.mul_(out, L.StackedVector(ctx, n).upload2(vh))
        ref = _AugTriRef(ax, e, ay)._op(vh)
        assert np.abs(out.download2() - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max())
        assert not np.any(out.download(out.hs - n, n))


def _chain_host(n, kappa):
    def lap(v):
        out = np.zeros_like(v)
        dv = v[1:] - v[:-1]
        out[:-1] -= dv
        out[1:] += dv
        return kappa * out
    return lap


@pytest.mark.parametrize("ball", [False, True])
def test_chain_objective_with_bounds_follows_the_oracle(dev_ctx, ball):
    """ChainSeparableLinear under the four-way box bounds (ball=False) and under ball + box (the slack form of src/optimize.jl:13-71) through
    `optimize`: every truncated-Newton solve reaches lfpsqp_projcg_tridiag with a stacked basis and is solved there (no -5), and the trajectory
    is the oracle's with hess_lag_vec! a matrix-free tridiagonal product.  Bounds that end up active make the trajectory sensitive to the last
    bit (squared slacks, tests/test_bounds_only.py): the oracle is run a second time from one ulp away and every iterate must stay within
    max(1e-10, 10 x that sensitivity); counts and step types must be equal throughout."""
    ctx = dev_ctx
    emu = _is_emu(ctx)
    n, m = (260, 4) if emu else (6000, 16)
    maxiter = 4 if emu else 10
    kind, kappa = 1, 1.7
    a = 0.5 + synth.hash_vector(21, n) ** 2
    c = 1.3 * synth.hash_vector(22, n)                                 # targets beyond the +-1 bounds on part of the rows
    phi, d1, d2 = _sep_host(kind, a, c)
    lap = _chain_host(n, kappa)
    P0 = synth.BallBoxProblem(n, m)
    x0 = 0.9 * synth.hash_vector(2, n) + 0.05
    f = lambda x: float(np.sum(phi(x[:n])) + 0.5 * np.dot(x[:n], lap(x[:n])))

    def grad_(g, x):
        g[:n] = d1(x[:n]) + lap(x[:n])

    par = dict(do_project_retract=False, maxiter=maxiter, tn_kappa=1e-6)

    def oracle(xs, trace):
        p = R.LFPSQPParams(disp=R.DisplayOption.off, **par)
        if ball:
            dv0 = P0.derivatives()

            def hlv_(dest, src, x, lam):
                dest[:] = (d2(x) + 2.0 * lam[m]) * src + lap(src)
            return R.optimize(f, P0.c_, P0.d_, xs, P0.xl, P0.xu, m, 1, p,
                              derivatives=R.Derivatives(grad_=grad_, hess_lag_vec_=hlv_, jac_c_=dv0.jac_c_, jac_d_=dv0.jac_d_), trace=trace)

        def hlv_(dest, src, x, lam):
            dest[:] = d2(x) * src + lap(src)
        return R.optimize(f, grad_, P0.eq.c_, P0.eq.jac_, hlv_, xs, P0.xl, P0.xu, m, p, trace=trace)

    tr0, tr1, tr = [], [], []
    xr, objr, lamr, tir = oracle(x0, tr0)
    oracle(np.nextafter(x0, np.inf), tr1)
    if ball:
        P = L.ChainSeparableLinear(ctx, n, m, ctx.matrix(n + 1, m + 1).hash_fill(1, 0, n, 1.0, n, m), P0.eq.b, kind, a, c, kappa=kappa,
                                   R2=P0.R2, xl=P0.xl, xu=P0.xu)
    else:
        P = L.ChainSeparableLinear(ctx, n, m, ctx.matrix(n, m).hash_fill(1), P0.eq.b, kind, a, c, kappa=kappa, xl=P0.xl, xu=P0.xu)
    import sys
    OPT = sys.modules["lfpsqp_jl_amd.optimize"]
    seen, rcs, orig = [], [], OPT.projcg_
    c_entry = ctx.L.lfpsqp_projcg_tridiag

    def spy(*args, **kw):
        seen.append((type(args[2]).__name__, type(args[3]).__name__))
        return orig(*args, **kw)

    def c_spy(*args):
        rc = c_entry(*args)
        rcs.append(rc)
        return rc
    OPT.projcg_ = spy
    ctx.L.lfpsqp_projcg_tridiag = c_spy
    try:
        x, obj, lam, ti = P.optimize(x0, L.LFPSQPParams(disp=L.DisplayOption.off, **par), trace=tr)
    finally:
        OPT.projcg_ = orig
        ctx.L.lfpsqp_projcg_tridiag = c_entry
    # every truncated-Newton solve: the tridiagonal operator over the stacked basis, on the C entry, which solved it
    assert seen and all(s == ("TridiagonalOperator", "InequalityDecompProject") for s in seen)
    assert len(rcs) == len(seen) and all(rc == 0 for rc in rcs)
    assert ti.iter == tir.iter and ti.condition.name == tir.condition.name and len(tr) == len(tr0)
    assert any((t.get('tn_iter') or 0) > 3 for t in tr0)
    sens = [np.linalg.norm(p['x'] - q['x']) / np.linalg.norm(q['x']) for p, q in zip(tr1, tr0)] + [np.inf] * (len(tr0) - len(tr1))
    dev = [np.linalg.norm(p['x'] - q['x']) / np.linalg.norm(q['x']) for p, q in zip(tr, tr0)]
    _note(f"chain objective with bounds (ball={ball}): deviation per outer iteration " + " ".join(f"{v:.1e}" for v in dev)
          + " | the oracle's own one-ulp sensitivity " + " ".join(f"{v:.1e}" for v in sens))
    for k, (p, q) in enumerate(zip(tr, tr0)):
        for key in ('tn_iter', 'steptype', 'rank', 'mtype', 'retract_iter1', 'ls_flag'):
            assert p.get(key) == q.get(key), (k, key, p.get(key), q.get(key))
        assert dev[k] <= max(1e-10, 10.0 * max(sens[:k + 1])), (k, dev[k], sens[k])
    assert abs(obj[-1] - objr[-1]) <= max(1e-10, 20.0 * max(sens)) * abs(objr[-1])
    assert np.linalg.norm(x - xr) <= max(1e-9, 10.0 * max(sens)) * np.linalg.norm(xr)
    active = np.sum(np.abs(x - P0.xl) < 1e-5) + np.sum(np.abs(x - P0.xu) < 1e-5)
    _note(f"chain objective with bounds (ball={ball}): {active} of {n} bounds active at the end")
    # DeviceOptions.tridiagonal_one_pass = False: the same operator through the callback path, the same trajectory
    ctx.options.tridiagonal_one_pass = False
    try:
        tr2 = []
        x2, obj2, lam2, ti2 = P.optimize(x0, L.LFPSQPParams(disp=L.DisplayOption.off, **par), trace=tr2)
    finally:
        ctx.options.tridiagonal_one_pass = True
    assert ti2.iter == ti.iter and [t.get('tn_iter') for t in tr2] == [t.get('tn_iter') for t in tr]
    dev2 = max(np.linalg.norm(p['x'] - q['x']) / np.linalg.norm(q['x']) for p, q in zip(tr2, tr))
    _note(f"chain objective with bounds (ball={ball}): one pass against the callback path, largest deviation {dev2:.1e}")
    assert dev2 <= max(1e-10, 10.0 * max(sens))


def test_stacked_tridiagonal_is_still_refused_where_the_one_pass_form_does_not_exist(dev_ctx):
    """With a stacked basis as with a plain one: a matrix view and two columns are LFPSQP_ERR_UNSUPPORTED (projcg_ then solves on the
    callback path); so is c != 0 with a stacked basis."""
    ctx = dev_ctx
    n = 900
    ax, ay = 4.0 * synth.hash_vector(3, n) + 5.0, 0.5 + synth.hash_vector(16, n) ** 2
    e = 0.8 * synth.hash_vector(15, n - 1)
    for m, view in ((2, False), (8, True)):
        P, P0, _, rank = _stacked_problem(ctx, n, m, False, view=view)
        A = _operator(ctx, n, ax, e, ay)
        bh = synth.hash_vector(4, 2 * n)
        tmp = np.zeros(n + m)
        R.mul_(tmp, R.adj(P0), bh)
        R.mul_(bh, P0, tmp, -1.0, 1.0)
        b = L.StackedVector(ctx, n).upload2(bh)
        rc, *_ = _solve_c(ctx, A, P, b, n, m, 1e-10)
        assert rc == -5
        x0, l0 = np.zeros(2 * n), np.zeros(n + m)
        i0, nr0 = R.projcg_(x0, l0, _AugTriRef(ax, e, ay), P0, bh, np.zeros(n + m), tol=1e-10)
        x, lam = L.StackedVector(ctx, n), ctx.vector(n + m)
        i1, nr1 = L.projcg_(x, lam, A, P, b, None, tol=1e-10, work=L.ProjCGWork(ctx, 0, m, stacked_N=n))
        assert i1 == i0 and np.linalg.norm(x.download2() - x0) <= 1e-10 * np.linalg.norm(x0)
    # c != 0 with a stacked basis
    P, P0, _, rank = _stacked_problem(ctx, n, 8, False)
    A = _operator(ctx, n, ax, e, ay)
    x, lam, Av = L.StackedVector(ctx, n), ctx.vector(n + 8), L.StackedVector(ctx, n)
    work = L.ProjCGWork(ctx, 0, 8, stacked_N=n)
    it, nr = _capi.c_i64(), C.c_double()
    a_c, u_c, w_c = A._c(), P._c(), work._c()
    cv, b = ctx.vector(8, np.ones(8)), L.StackedVector(ctx, n)
    rc = ctx.L.lfpsqp_projcg_tridiag(ctx.h, x.h, lam.h, C.byref(a_c), Av.h, C.byref(u_c), b.h, cv.h, 1e-10, 100, 2 * n, 0,
                                     C.byref(w_c), C.byref(it), C.byref(nr))
    assert rc == -5


def test_stacked_tridiagonal_refuses_row_shards(emu_lib):
    """A communicator (the row-shard case): the stacked one-pass solve and the stacked product answer LFPSQP_ERR_UNSUPPORTED."""
    ctx = L.Context(0, emu_lib)
    try:
        ctx.comm_init_callback(0, 1, lambda ptr, count, op, stream: 0)
        n, m = 700, 8
        P, P0, _, rank = _stacked_problem(ctx, n, m, False)
        A = _operator(ctx, n, 4.0 * synth.hash_vector(3, n) + 5.0, 0.8 * synth.hash_vector(15, n - 1), np.ones(n))
        b = L.StackedVector(ctx, n).upload2(synth.hash_vector(4, 2 * n))
        rc, *_ = _solve_c(ctx, A, P, b, n, m, 1e-10)
        assert rc == -5
        a_c, out = A._c(), L.StackedVector(ctx, n)
        assert ctx.L.lfpsqp_tridiag_mul(ctx.h, C.byref(a_c), b.h, out.h) == -5
    finally:
        ctx.close()
