"""projcg! with a BANDED Hessian (bandwidth 2 .. 4) on the one-pass iteration (lfpsqp_projcg_band).

A penalty on second or higher differences -- Whittaker / Hodrick-Prescott smoothing, curvature terms -- gives a pentadiagonal or wider
Lagrangian Hessian, which the reference applies as a LinearMap (src/optimize.jl:228-230).  The banded entry keeps the tridiagonal path's ONE
pass per iteration: the row record of the pass is the same, the preparation kernel reads d within 2 bw rows, and U'A U takes one shifted Gram
pass per off-diagonal (include/lfpsqp_hip.h).  Checked here against numpy and the oracle's projcg! with the same operator as a matrix-free map:
the product (plain, stacked, ignored tail entries poisoned), counts / iterates / multipliers for dominant and non-dominant couplings, c != 0,
the iteration limit, negative curvature, materialised and factored bases, the callback path, bw = 1 against the tridiagonal entry bit for
bit, the stacked form under four-way bounds, ChainSeparableLinear(order = 2, 3) through `optimize`, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import lfpsqp_jl_amd as L
from lfpsqp_jl_amd import _capi
from oracle import lfpsqp_ref as R
from oracle import synth

from .test_capi_retractions import _compare_traces, _is_emu, _note, _sep_host
from .test_tridiag_bounds import _stacked_problem

POISON = 123.0


def _band(v, a, offs):
    """(A v) = a v + sum_k (off_k[i-k] v_{i-k} + off_k[i] v_{i+k}) over len(a) rows; offs[k-1] holds the n - k used couplings."""
    n = len(a)
    out = a * v[:n]
    for k, e in enumerate(offs, start=1):
        if n > k:
            out[:n - k] += e * v[k:n]
            out[k:n] += e * v[:n - k]
    return out


class _BandRef:
    def __init__(self, a, offs, ay=None):
        self.a, self.offs, self.ay = a, offs, ay

    def _op(self, v):
        if self.ay is None:
            return _band(v, self.a, self.offs)
        n = len(self.a)
        return np.concatenate([_band(v[:n], self.a, self.offs), self.ay * v[n:]])

    def mul_(self, dest, v, al=None, be=None):
        t = self._op(v)
        dest[:] = t if al is None else al * t + be * dest
        return dest

    def adjoint(self):
        return self


def _offs(n, bw, scale, seed=15):
    return [scale / k * synth.hash_vector(seed + k, max(n - k, 1))[:max(n - k, 0)] for k in range(1, bw + 1)]


def _off_matrix(ctx, n, offs, extra_cols=0):
    """N x (bw + extra) device matrix, column k-1 = off_k with its ignored tail (rows i + k >= n) and any extra column poisoned."""
    bw = len(offs)
    M = np.full((n, bw + extra_cols), POISON, order='F')
    for k, e in enumerate(offs, start=1):
        M[:len(e), k - 1] = e
    return ctx.matrix(n, bw + extra_cols, M)


def _operator(ctx, a, offs, a0=0.0, ay=None):
    n = len(a)
    if ay is None:
        dg = ctx.vector(n, a - a0)
    else:
        dg = L.StackedVector(ctx, n).upload2(np.concatenate([a, ay]) - a0)
    return L.BandedOperator(a0, dg, _off_matrix(ctx, n, offs, extra_cols=1), len(offs))


@pytest.mark.parametrize("bw", [2, 3, 4])
def test_banded_product(dev_ctx, bw):
    ctx = dev_ctx
    for n in sorted({1, 2, 3, bw, bw + 1, 511, 2048, 2049, 4097}):
        a = 4.0 * synth.hash_vector(3, n) + 5.0
        offs = _offs(n, bw, 0.8)
        vh = synth.hash_vector(7, n)
        A = _operator(ctx, a, offs, a0=0.25)
        out = ctx.vector(n)
        A.mul_(out, ctx.vector(n, vh))
        ref = _band(vh, a, offs)
        assert np.abs(out.download() - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max()), n
        out.upload(np.ones(n))
        A.mul_(out, ctx.vector(n, vh), 2.0, -1.0)                   # mul!(dest, A, v, alpha, beta)
        assert np.abs(out.download() - (2.0 * ref - 1.0)).max() <= 1e-13 * max(1.0, np.abs(ref).max()), n
        # stacked pair: the couplings on the x half, the y half diagonal, the gap left at zero
        ay = synth.hash_vector(16, n)
        vs = synth.hash_vector(8, 2 * n)
        As = _operator(ctx, a, offs, a0=0.25, ay=ay)
        outs = L.StackedVector(ctx, n)
        As.mul_(outs, L.StackedVector(ctx, n).upload2(vs))
        refs = _BandRef(a, offs, ay)._op(vs)
        assert np.abs(outs.download2() - refs).max() <= 1e-14 * max(1.0, np.abs(refs).max()), n
        assert not np.any(outs.download(outs.hs - n, n))


def _basis(ctx, n, m, factored):
    if factored:                                   # the basis kept as U = J W (lfpsqp_basis.Z == NULL)
        Jh = synth.hash_matrix(5, n, m)
        J = ctx.matrix(n, m, np.asfortranarray(Jh))
        W = np.zeros((m, m), order='F')
        S, Vt, rank = L.ksvd_(J, None, W=W)
        return L.DeviceBasis(None, rank, generator=(J, W)), np.asfortranarray(Jh @ W)
    Uh, _ = np.linalg.qr(synth.hash_matrix(1, n, m))
    Uh = np.asfortranarray(Uh)
    return L.DeviceBasis(ctx.matrix(n, m, Uh)), Uh


def _dense(a, offs):
    A = np.diag(a)
    for k, e in enumerate(offs, start=1):
        A += np.diag(e, k) + np.diag(e, -k)
    return A


# (bw, n, m, factored, dominant): n at and off multiples of 16 and of 2048; m from a narrow tile to past a tile width
_CASES = [(2, 1500, 6, False, True), (4, 1700, 130, False, False), (2, 2048, 128, False, False), (4, 4096, 33, True, True),
          (2, 2400, 128, True, False), (4, 800, 300, False, True)]


@pytest.mark.parametrize("bw,n,m,factored,dominant", _CASES)
def test_projcg_with_a_banded_operator_on_one_pass(dev_ctx, bw, n, m, factored, dominant):
    ctx = dev_ctx
    a = 4.0 * synth.hash_vector(3, n) + 5.0
    offs = _offs(n, bw, 0.8 if dominant else 3.0)                    # both signs
    if not dominant:
        a = a + 5.0                                                  # positive definite (checked) but not diagonally dominant: negative Gram weights
        c = a - sum(np.abs(np.concatenate([e, np.zeros(k)])) + np.abs(np.concatenate([np.zeros(k), e])) for k, e in enumerate(offs, start=1))
        assert np.any(c < 0)
        assert np.linalg.eigvalsh(_dense(a, offs))[0] > 0.05
    U, Uh = _basis(ctx, n, m, factored)
    A = _operator(ctx, a, offs)
    Aref = _BandRef(a, offs)
    bh = synth.hash_vector(4, n)
    b = ctx.vector(n, bh)
    work = L.ProjCGWork(ctx, n, m)
    for ch, tol in ((None, 1e-10), (np.linspace(-1, 1, m), 1e-12)):
        x0, l0 = np.zeros(n), np.zeros(m)
        i0, nr0 = R.projcg_(x0, l0, Aref, Uh, bh, np.zeros(m) if ch is None else ch, tol=tol)
        x, lam = ctx.vector(n), ctx.vector(m)
        i1, nr1 = L.projcg_(x, lam, A, U, b, None if ch is None else ctx.vector(m, ch), tol=tol, work=work)
        dx = np.linalg.norm(x.download() - x0) / np.linalg.norm(x0)
        print(f"[band] bw={bw} n={n} m={m} factored={factored} dominant={dominant}: iterations {i1} (oracle {i0}), x {dx:.1e}")
        assert i1 == i0 and i1 > 3 and nr1 == pytest.approx(nr0, rel=1e-5)
        assert dx <= 1e-10
        assert np.abs(lam.download() - l0).max() <= 1e-10
        if factored:
            continue                               # (the callback path needs a materialised basis)
        A.fused = False                            # the callback path (lfpsqp_projcg_op, two passes per iteration) with the same operator
        x2, lam2 = ctx.vector(n), ctx.vector(m)
        i2, nr2 = L.projcg_(x2, lam2, A, U, b, None if ch is None else ctx.vector(m, ch), tol=tol)
        A.fused = True
        assert i2 == i1
        assert np.linalg.norm(x.download() - x2.download()) <= 1e-10 * np.linalg.norm(x0)
    # the iteration limit (src/projcg.jl:71)
    x0, l0 = np.zeros(n), np.zeros(m)
    i0, nr0 = R.projcg_(x0, l0, Aref, Uh, bh, np.zeros(m), tol=1e-30, maxit=5)
    x, lam = ctx.vector(n), ctx.vector(m)
    i1, nr1 = L.projcg_(x, lam, A, U, b, None, tol=1e-30, maxit=5, work=work)
    assert (i1, i0) == (5, 5) and nr1 == pytest.approx(nr0, rel=1e-9)
    assert np.linalg.norm(x.download() - x0) <= 1e-12 * np.linalg.norm(x0)
    # negative curvature (src/projcg.jl:77-82)
    x0, l0 = np.zeros(n), np.zeros(m)
    i0, nr0 = R.projcg_(x0, l0, _BandRef(-a, offs), Uh, bh, np.zeros(m), tol=1e-10)
    x, lam = ctx.vector(n), ctx.vector(m)
    i1, nr1 = L.projcg_(x, lam, _operator(ctx, -a, offs), U, b, None, tol=1e-10, work=work)
    assert (i1, nr1) == (i0, nr0) and math.isinf(nr1)
    assert np.linalg.norm(x.download() - x0) <= 1e-10 and np.all(np.isnan(lam.download()))


def test_bandwidth_one_is_the_tridiagonal_path(dev_ctx):
    """lfpsqp_projcg_band with one off-diagonal runs the kernels of lfpsqp_projcg_tridiag: x, lambda, the count and nr bit for bit, over a plain
    and over a stacked basis."""
    ctx = dev_ctx
    n, m = 2049, 33
    a = 4.0 * synth.hash_vector(3, n) + 5.0
    e = 3.0 * synth.hash_vector(15, n - 1)
    a = a + 2.5                                                      # (not diagonally dominant: the negative-weight Gram pass runs too)
    U, Uh = _basis(ctx, n, m, False)
    bh = synth.hash_vector(4, n)
    b = ctx.vector(n, bh)
    res = []
    for A in (L.TridiagonalOperator(0.5, ctx.vector(n, a - 0.5), ctx.vector(n, np.concatenate([e, [POISON]]))), _operator(ctx, a, [e], a0=0.5)):
        x, lam = ctx.vector(n), ctx.vector(m)
        it, nr = L.projcg_(x, lam, A, U, b, ctx.vector(m, np.linspace(-1, 1, m)), tol=1e-12, work=L.ProjCGWork(ctx, n, m))
        res.append((it, nr, x.download().tobytes(), lam.download().tobytes()))
    assert res[0][0] > 3 and res[0] == res[1]
    # stacked
    P, P0, _, rank = _stacked_problem(ctx, n, m, False)
    ay = 0.5 + synth.hash_vector(16, n) ** 2
    bs = synth.hash_vector(4, 2 * n)
    tmp = np.zeros(n + m)
    R.mul_(tmp, R.adj(P0), bs)
    R.mul_(bs, P0, tmp, -1.0, 1.0)
    b2 = L.StackedVector(ctx, n).upload2(bs)
    dg = L.StackedVector(ctx, n).upload2(np.concatenate([a, ay]))
    res = []
    for A in (L.TridiagonalOperator(0.0, dg, ctx.vector(n, np.concatenate([e, [POISON]]))), L.BandedOperator(0.0, dg, _off_matrix(ctx, n, [e]), 1)):
        x, lam = L.StackedVector(ctx, n), ctx.vector(n + m)
        it, nr = L.projcg_(x, lam, A, P, b2, None, tol=1e-12, work=L.ProjCGWork(ctx, 0, m, stacked_N=n))
        res.append((it, nr, x.download2().tobytes(), lam.download().tobytes()))
    assert res[0][0] > 3 and res[0] == res[1]


def _solve_stacked_c(ctx, A, P, b, n, m, tol, maxit=None):
    """lfpsqp_projcg_band itself over a stacked basis (no fall-back): rc, iterations, nr, x, lambda."""
    x, lam = L.StackedVector(ctx, n), ctx.vector(n + m)
    work = L.ProjCGWork(ctx, 0, m, stacked_N=n)
    Av = L.StackedVector(ctx, n)
    it, nr = _capi.c_i64(), C.c_double()
    u_c, w_c = P._c(), work._c()
    rc = ctx.L.lfpsqp_projcg_band(ctx.h, x.h, lam.h, A.a0, A.dg.h, A.off.h, A.bw, Av.h, C.byref(u_c), b.h, None, float(tol),
                                  int(2 * n + m if maxit is None else maxit), 2 * n, 1, C.byref(w_c), C.byref(it), C.byref(nr))
    return rc, it.value, nr.value, x, lam


@pytest.mark.parametrize("bw,n,m,factored", [(2, 2049, 16, False), (3, 2048, 128, True), (3, 1500, 33, False)])
def test_stacked_banded_solver_follows_the_oracle(dev_ctx, bw, n, m, factored):
    """Four-way bounds: lfpsqp_projcg_band over a stacked basis against the oracle's projcg! with the augmented map blockdiag(T, diag(ay))."""
    ctx = dev_ctx
    P, P0, _, rank = _stacked_problem(ctx, n, m, factored)
    assert rank == m
    ax = 4.0 * synth.hash_vector(3, n) + 9.0
    offs = _offs(n, bw, 2.0)
    ay = 0.5 + synth.hash_vector(16, n) ** 2
    A = _operator(ctx, ax, offs, ay=ay)
    Aref = _BandRef(ax, offs, ay)
    bh = synth.hash_vector(4, 2 * n)
    tmp = np.zeros(n + m)
    R.mul_(tmp, R.adj(P0), bh)
    R.mul_(bh, P0, tmp, -1.0, 1.0)                                      # a right-hand side in the tangent space, like optimize's d
    b = L.StackedVector(ctx, n).upload2(bh)
    for tol, maxit in ((1e-10, None), (1e-300, 5)):
        x0, l0 = np.zeros(2 * n), np.zeros(n + m)
        i0, nr0 = R.projcg_(x0, l0, Aref, P0, bh, np.zeros(n + m), tol=tol, maxit=maxit)
        rc, i1, nr1, x, lam = _solve_stacked_c(ctx, A, P, b, n, m, tol, maxit)
        assert rc == 0
        xd, ld = x.download2(), lam.download()
        dx_ = np.linalg.norm(xd - x0) / np.linalg.norm(x0)
        dl_ = np.abs(ld - l0).max() / np.abs(l0).max()
        print(f"[stacked band] bw={bw} n={n} m={m} factored={factored} maxit={maxit}: iterations {i1} (oracle {i0}), x {dx_:.1e}, lambda {dl_:.1e}")
        assert i1 == i0 and (maxit is not None or i1 > 3)
        assert nr1 == pytest.approx(nr0, rel=1e-6)
        assert dx_ <= 1e-10 and dl_ <= 1e-9
        if factored:
            continue
        A.fused = False
        x2, lam2 = L.StackedVector(ctx, n), ctx.vector(n + m)
        i2, nr2 = L.projcg_(x2, lam2, A, P, b, None, tol=tol, maxit=maxit, work=L.ProjCGWork(ctx, 0, m, stacked_N=n))
        A.fused = True
        assert i2 == i1 and np.linalg.norm(x2.download2() - xd) <= 1e-10 * np.linalg.norm(x0)
    # negative curvature
    x0, l0 = np.zeros(2 * n), np.zeros(n + m)
    i0, nr0 = R.projcg_(x0, l0, _BandRef(-ax, offs, ay), P0, bh, np.zeros(n + m), tol=1e-10)
    rc, i1, nr1, x, lam = _solve_stacked_c(ctx, _operator(ctx, -ax, offs, ay=ay), P, b, n, m, 1e-10)
    assert rc == 0 and (i1, nr1) == (i0, nr0) and math.isinf(nr1)
    assert np.all(np.isnan(lam.download()))


def _diff_host(n, order, kappa):
    def pen(v):                                                         # kappa D'D v, D the order-th forward difference
        return kappa * (-1) ** order * np.diff(np.concatenate([np.zeros(order), np.diff(v, order), np.zeros(order)]), order)
    return pen


@pytest.mark.parametrize("order,cons", [(2, "eq"), (3, "eq"), (2, "box"), (3, "box"), (2, "ballbox"), (3, "ballbox")])
def test_chain_objective_of_higher_order_follows_the_oracle(dev_ctx, order, cons):
    """ChainSeparableLinear(order = 2, 3): f = sum phi(x_i) + kappa/2 ||D^order x||^2 through `optimize`.  Every truncated-Newton solve runs a
    BandedOperator from the tangent step's state on lfpsqp_projcg_band, and the trajectory is the oracle's with hess_lag_vec! built from
    np.diff.  Under bounds the oracle is run a second time from one ulp away, as in tests/test_tridiag_bounds.py."""
    ctx = dev_ctx
    emu = _is_emu(ctx)
    n, m = (260, 4) if emu else (6000, 16)
    maxiter = 4 if emu else 10
    kind, kappa = 1, 0.9
    a = 0.5 + synth.hash_vector(21, n) ** 2
    c = (1.3 if cons != "eq" else 0.3) * synth.hash_vector(22, n)
    phi, d1, d2 = _sep_host(kind, a, c)
    pen = _diff_host(n, order, kappa)
    v = synth.hash_vector(30, n)
    H = np.array([pen(col) for col in np.eye(min(n, 40))])             # (the penalty is kappa D'D: a spot check on a small section)
    D = np.diff(np.eye(min(n, 40)), order, axis=0)
    assert np.allclose(H, kappa * D.T @ D) and abs(v @ pen(v) - kappa * np.sum(np.diff(v, order) ** 2)) <= 1e-10 * abs(v @ pen(v))
    P0 = synth.BallBoxProblem(n, m)
    x0 = (0.9 * synth.hash_vector(2, n) + 0.05) if cons != "eq" else synth.hash_vector(2, n)
    f = lambda x: float(np.sum(phi(x[:n])) + 0.5 * np.sum(kappa * np.diff(x[:n], order) ** 2))

    def grad_(g, x):
        g[:n] = d1(x[:n]) + pen(x[:n])

    par = dict(do_project_retract=False, maxiter=maxiter, tn_kappa=1e-6)

    def oracle(xs, trace):
        p = R.LFPSQPParams(disp=R.DisplayOption.off, **par)
        if cons == "ballbox":
            dv0 = P0.derivatives()

            def hlv_(dest, src, x, lam):
                dest[:] = (d2(x) + 2.0 * lam[m]) * src + pen(src)
            return R.optimize(f, P0.c_, P0.d_, xs, P0.xl, P0.xu, m, 1, p,
                              derivatives=R.Derivatives(grad_=grad_, hess_lag_vec_=hlv_, jac_c_=dv0.jac_c_, jac_d_=dv0.jac_d_), trace=trace)

        def hlv_(dest, src, x, lam):
            dest[:] = d2(x) * src + pen(src)
        xl, xu = (None, None) if cons == "eq" else (P0.xl, P0.xu)
        return R.optimize(f, grad_, P0.eq.c_, P0.eq.jac_, hlv_, xs, xl, xu, m, p, trace=trace)

    tr0, tr1, tr = [], [], []
    xr, objr, lamr, tir = oracle(x0, tr0)
    sens = [0.0]
    if cons != "eq":
        oracle(np.nextafter(x0, np.inf), tr1)
        sens = [np.linalg.norm(p['x'] - q['x']) / np.linalg.norm(q['x']) for p, q in zip(tr1, tr0)] + [np.inf] * (len(tr0) - len(tr1))
    if cons == "ballbox":
        P = L.ChainSeparableLinear(ctx, n, m, ctx.matrix(n + 1, m + 1).hash_fill(1, 0, n, 1.0, n, m), P0.eq.b, kind, a, c, kappa=kappa,
                                   order=order, R2=P0.R2, xl=P0.xl, xu=P0.xu)
    elif cons == "box":
        P = L.ChainSeparableLinear(ctx, n, m, ctx.matrix(n, m).hash_fill(1), P0.eq.b, kind, a, c, kappa=kappa, order=order, xl=P0.xl, xu=P0.xu)
    else:
        P = L.ChainSeparableLinear(ctx, n, m, ctx.matrix(n, m).hash_fill(1), P0.eq.b, kind, a, c, kappa=kappa, order=order)
    assert not hasattr(P, "offdiag") and P.offdiags.m == order
    import sys
    OPT = sys.modules["lfpsqp_jl_amd.optimize"]
    seen, rcs, orig = [], [], OPT.projcg_
    c_entry = ctx.L.lfpsqp_projcg_band

    def spy(*args, **kw):
        seen.append((type(args[2]).__name__, bool(kw.get("start_given"))))
        return orig(*args, **kw)

    def c_spy(*args):
        rc = c_entry(*args)
        rcs.append(rc)
        return rc
    OPT.projcg_ = spy
    ctx.L.lfpsqp_projcg_band = c_spy
    try:
        x, obj, lam, ti = P.optimize(x0, L.LFPSQPParams(disp=L.DisplayOption.off, **par), trace=tr)
    finally:
        OPT.projcg_ = orig
        ctx.L.lfpsqp_projcg_band = c_entry
    assert seen and all(s == ("BandedOperator", True) for s in seen)
    assert len(rcs) == len(seen) and all(rc == 0 for rc in rcs)
    assert ti.iter == tir.iter and ti.condition.name == tir.condition.name
    print(f"[chain order {order} {cons}] Newton-system iterations", [t.get('tn_iter') for t in tr0])
    # (with the ball its multiplier adds 2 lam to the diagonal and the solves are shorter: more than two iterations there)
    assert any((t.get('tn_iter') or 0) > (2 if cons == "ballbox" else 3) for t in tr0)
    rtol = max(1e-10, 10.0 * max(sens))
    _note(f"chain objective of order {order} ({cons}): the oracle's one-ulp sensitivity {max(sens):.1e}")
    assert _compare_traces(tr, tr0, rtol=rtol) is None
    assert abs(obj[-1] - objr[-1]) <= max(1e-11, 20.0 * max(sens)) * abs(objr[-1])
    assert np.linalg.norm(x - xr) <= max(1e-9, 10.0 * max(sens)) * np.linalg.norm(xr)
    # DeviceOptions.tridiagonal_one_pass = False: the same operator through the callback path, the same trajectory
    ctx.options.tridiagonal_one_pass = False
    try:
        tr2 = []
        x2, obj2, lam2, ti2 = P.optimize(x0, L.LFPSQPParams(disp=L.DisplayOption.off, **par), trace=tr2)
    finally:
        ctx.options.tridiagonal_one_pass = True
    assert ti2.iter == ti.iter and _compare_traces(tr2, tr0, rtol=rtol) is None


def test_banded_operator_is_refused_where_the_one_pass_form_does_not_exist(dev_ctx):
    """bw outside 1 .. 4 is an argument error; a matrix view as basis and two columns are LFPSQP_ERR_UNSUPPORTED, and projcg_ then solves on the
    callback path."""
    ctx = dev_ctx
    n = 900
    a = 4.0 * synth.hash_vector(3, n) + 5.0
    offs = _offs(n, 2, 0.8)
    A = _operator(ctx, a, offs)
    Aref = _BandRef(a, offs)
    bh = synth.hash_vector(4, n)
    b = ctx.vector(n, bh)
    for m, view in ((2, False), (8, True), (8, False)):
        Uh, _ = np.linalg.qr(synth.hash_matrix(1, n, m))
        Uh = np.asfortranarray(Uh)
        Zd = ctx.matrix(n, m, Uh)
        U = L.DeviceBasis(Zd.view(ctx.vector(n, np.ones(n))) if view else Zd)
        x, lam, Av = ctx.vector(n), ctx.vector(m), ctx.vector(n)
        work = L.ProjCGWork(ctx, n, m)
        it, nr = _capi.c_i64(), C.c_double()
        u_c, w_c = U._c(), work._c()
        for bw in (0, 5):
            assert ctx.L.lfpsqp_projcg_band(ctx.h, x.h, lam.h, 0.0, A.dg.h, A.off.h, bw, Av.h, C.byref(u_c), b.h, None, 1e-10, 100, n, 1,
                                            C.byref(w_c), C.byref(it), C.byref(nr)) == -1
            assert ctx.L.lfpsqp_band_mul(ctx.h, 0.0, A.dg.h, A.off.h, bw, b.h, Av.h) == -1
        if not view and m == 8:
            continue
        rc = ctx.L.lfpsqp_projcg_band(ctx.h, x.h, lam.h, 0.0, A.dg.h, A.off.h, 2, Av.h, C.byref(u_c), b.h, None, 1e-10, 100, n, 1,
                                      C.byref(w_c), C.byref(it), C.byref(nr))
        assert rc == -5
        x0, l0 = np.zeros(n), np.zeros(m)
        i0, nr0 = R.projcg_(x0, l0, Aref, Uh, bh, np.zeros(m), tol=1e-10)
        x, lam = ctx.vector(n), ctx.vector(m)
        i1, nr1 = L.projcg_(x, lam, A, U, b, None, tol=1e-10, work=work)
        assert i1 == i0 and np.linalg.norm(x.download() - x0) <= 1e-10 * np.linalg.norm(x0)
    # a view as the couplings
    offv = A.off.view(ctx.vector(n, np.ones(n)))
    assert ctx.L.lfpsqp_band_mul(ctx.h, 0.0, A.dg.h, offv.h, 2, b.h, Av.h) == -1


def test_banded_operator_refuses_row_shards(emu_lib):
    """A communicator (the row-shard case): the one-pass solve and the product answer LFPSQP_ERR_UNSUPPORTED; projcg_ raises."""
    ctx = L.Context(0, emu_lib)
    try:
        ctx.comm_init_callback(0, 1, lambda ptr, count, op, stream: 0)
        n, m = 700, 8
        a = 4.0 * synth.hash_vector(3, n) + 5.0
        A = _operator(ctx, a, _offs(n, 3, 0.8))
        Uh, _ = np.linalg.qr(synth.hash_matrix(1, n, m))
        U = L.DeviceBasis(ctx.matrix(n, m, np.asfortranarray(Uh)))
        b, x, lam, Av = ctx.vector(n, synth.hash_vector(4, n)), ctx.vector(n), ctx.vector(m), ctx.vector(n)
        work = L.ProjCGWork(ctx, n, m)
        it, nr = _capi.c_i64(), C.c_double()
        u_c, w_c = U._c(), work._c()
        rc = ctx.L.lfpsqp_projcg_band(ctx.h, x.h, lam.h, 0.0, A.dg.h, A.off.h, 3, Av.h, C.byref(u_c), b.h, None, 1e-10, 100, n, 1,
                                      C.byref(w_c), C.byref(it), C.byref(nr))
        assert rc == -5
        assert ctx.L.lfpsqp_band_mul(ctx.h, 0.0, A.dg.h, A.off.h, 3, b.h, Av.h) == -5
        with pytest.raises(L.LfpsqpError):
            L.projcg_(x, lam, A, U, b, None, tol=1e-10, work=work)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_banded_projcg_at_protocol_size(gpu_lib):
    """(1e6, 128), bw = 2, not diagonally dominant: equal counts and iterates within 1e-10 of the oracle."""
    ctx = L.Context(0, gpu_lib)
    try:
        n, m = 1_000_000, 128
        a = 4.0 * synth.hash_vector(3, n) + 10.0
        offs = _offs(n, 2, 3.0)
        U, Uh = _basis(ctx, n, m, False)
        bh = synth.hash_vector(4, n)
        x0, l0 = np.zeros(n), np.zeros(m)
        i0, nr0 = R.projcg_(x0, l0, _BandRef(a, offs), Uh, bh, np.zeros(m), tol=1e-10)
        x, lam = ctx.vector(n), ctx.vector(m)
        i1, nr1 = L.projcg_(x, lam, _operator(ctx, a, offs), U, ctx.vector(n, bh), None, tol=1e-10, work=L.ProjCGWork(ctx, n, m))
        dx = np.linalg.norm(x.download() - x0) / np.linalg.norm(x0)
        print(f"[band 1e6] iterations {i1} (oracle {i0}), x {dx:.1e}")
        assert i1 == i0 and i1 > 3 and dx <= 1e-10 and np.abs(lam.download() - l0).max() <= 1e-10
    finally:
        ctx.close()
