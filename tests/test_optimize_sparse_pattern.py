"""`optimize` with a SparseLagrangianHessian: the structure / values interface from the public entry down to lfpsqp_sphess_set_values.

The problem is one lfpsqp_sphess_edge_eval cannot express: f(x) = sum_i phi(x_i) + kappa sum_e w_e softplus(x_i + x_j) over the edges of a test
graph (off-diagonal Hessian entries kappa w_e sigma'(x_i + x_j) > 0, a function of the SUM of the endpoints), under linear equalities A x = b and
the nonlinear equality x'x = r^2, whose multiplier enters the diagonal triplets: values_ depends on lam.  Every derivative is a host callback.
The triplet list: the edges (every other one mirrored), and on the diagonal phi''(x_i) once per row, 2 lam_q once per row, and kappa w_e sigma'
once per END of every edge -- chains of up to row degree + 2 diagonal duplicates.

Reference: the oracle's R.optimize with a matrix-free hess_lag_vec! built from the SAME triplets by np.bincount.  Bar: equal iteration counts,
step types and flags, iterates within 1e-10 relative (_compare_traces).  Whether a truncated-Newton exit sits near its tolerance is decided on the
oracle alone, by the rule of tests/test_projcg_sparse.py::test_graph_objective_follows_the_oracle: the oracle is run a second time from one ulp
away and must reproduce its own counts with iterates within 1e-12 -- a starting point whose exits were borderline would not."""
import sys

import numpy as np
import pytest

import lfpsqp_jl_amd as L
from oracle import lfpsqp_ref as R
from oracle import synth

from .test_capi_retractions import _compare_traces, _note, _sep_host
from .test_projcg_sparse import KAPPA, _graph

ML = 4                                                              # linear equalities; m = ML + 1
_PAR = dict(do_project_retract=False, maxiter=4, tn_kappa=1e-6)


class _Problem:
    def __init__(self, name):
        self.name = name
        self.n, self.ei, self.ej = n, ei, ej = _graph(name)
        E = len(ei)
        self.w = 0.5 + synth.hash_vector(41, E) ** 2
        self.phi, self.d1, self.d2 = _sep_host(1, 0.5 + synth.hash_vector(21, n) ** 2, 1.3 * synth.hash_vector(22, n))
        self.A = np.asfortranarray(synth.hash_matrix(1, n, ML).T) - 0.5
        self.x0 = 0.9 * synth.hash_vector(2, n) + 0.05
        self.b = self.A @ self.x0
        self.r2 = float(self.x0 @ self.x0)                          # (x0 is feasible)
        self.m = ML + 1
        self.q = 0.3 * (synth.hash_vector(23, n) - 0.5)             # the inequality d(x) = q'x - beta
        self.beta = float(self.q @ self.x0) + 0.4
        mirror = np.arange(E) % 2 == 1
        ar = np.arange(n)
        self.rows = np.concatenate([np.where(mirror, ej, ei), ar, ei, ar, ej])
        self.cols = np.concatenate([np.where(mirror, ei, ej), ar, ei, ar, ej])
        self.calls = dict(values=0, hlv=0)

    def sig(self, x):
        return 1.0 / (1.0 + np.exp(-(x[self.ei] + x[self.ej])))

    def f(self, x):
        n = self.n
        return float(np.sum(self.phi(x[:n])) + KAPPA * np.sum(self.w * np.logaddexp(0.0, x[self.ei] + x[self.ej])))

    def grad_(self, g, x):
        n = self.n
        s = KAPPA * self.w * self.sig(x)
        g[:n] = self.d1(x[:n]) + np.bincount(self.ei, s, n) + np.bincount(self.ej, s, n)

    def c_(self, cval, x):
        cval[:ML] = self.A @ x[:self.n] - self.b
        cval[ML] = x[:self.n] @ x[:self.n] - self.r2
        return cval

    def jac_c_(self, J, cval, x):
        self.c_(cval, x)
        J[:ML, :] = self.A
        J[ML, :] = 2.0 * x[:self.n]

    def d_(self, dval, x):
        dval[0] = self.q @ x[:self.n] - self.beta
        return dval

    def jac_d_(self, J, dval, x):
        self.d_(dval, x)
        J[0, :] = self.q

    def _values(self, vals, x, lam):
        n, E = self.n, len(self.ei)
        s = self.sig(x)
        h = KAPPA * self.w * s * (1.0 - s)
        vals[:E] = h
        vals[E:E + n] = self.d2(x[:n])
        vals[E + n:2 * E + n] = h
        vals[2 * E + n:2 * E + 2 * n] = 2.0 * lam[ML]
        vals[2 * E + 2 * n:] = h

    def values_(self, vals, x, lam):
        assert vals.shape == (len(self.rows),) and x.shape == (self.n,)
        self.calls["values"] += 1
        self._values(vals, x, lam)

    def hlv_(self, dest, src, x, lam):
        """Matrix-free, from the same triplets: a triplet (r, c, v) adds v src_c to dest_r, and v src_r to dest_c when r != c."""
        self.calls["hlv"] += 1
        n = self.n
        vals = np.empty(len(self.rows))
        self._values(vals, x, lam)
        off = self.rows != self.cols
        dest[:n] = np.bincount(self.rows, vals * src[self.cols], n) + np.bincount(self.cols[off], vals[off] * src[self.rows[off]], n)

    def box(self):
        return self.x0 - 0.5 - 0.25 * synth.hash_vector(24, self.n), self.x0 + 0.5 + 0.25 * synth.hash_vector(25, self.n)

    def args(self, form):
        xl, xu = self.box()
        if form == "eq":
            return (self.f, self.c_, self.x0, self.m)
        if form == "box":
            return (self.f, self.c_, self.x0, xl, xu, self.m)
        if form == "slack8":
            return (self.f, self.c_, self.d_, self.x0, None, None, self.m, 1)
        return (self.f, self.c_, self.d_, np.array([-1.0]), np.array([0.6]), self.x0, xl, xu, self.m, 1)


_PROBLEMS, _ORACLE = {}, {}


def _problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = _Problem(name)
    return _PROBLEMS[name]


def _oracle(name, form):
    """The oracle's run and its run from one ulp away; once per case, shared by the emulator and GPU runs, read-only."""
    if (name, form) not in _ORACLE:
        P = _problem(name)
        dv = R.Derivatives(grad_=P.grad_, hess_lag_vec_=P.hlv_, jac_c_=P.jac_c_, jac_d_=P.jac_d_)
        runs = []
        for shift in (False, True):
            args = list(P.args(form))
            k = [i for i, a in enumerate(args) if a is P.x0][0]
            if shift:
                args[k] = np.nextafter(P.x0, np.inf)
            tr = []
            x, obj, lam, ti = R.optimize(*args, R.LFPSQPParams(disp=R.DisplayOption.off, **_PAR), derivatives=dv, trace=tr)
            runs.append((tr, x, obj, ti))
        tr0, tr1 = runs[0][0], runs[1][0]
        sens = [np.linalg.norm(p['x'] - q['x']) / np.linalg.norm(q['x']) for p, q in zip(tr1, tr0)] + [np.inf] * (len(tr0) - len(tr1))
        same = all(p.get(k) == q.get(k) for p, q in zip(tr1, tr0) for k in ('tn_iter', 'steptype', 'alpha', 'ls_flag'))
        _ORACLE[(name, form)] = runs[0] + (max(sens), same)
    return _ORACLE[(name, form)]


def _device_run(ctx, P, form, pattern, one_pass=True):
    """optimize on the device with the pattern form (as Derivatives fields, or as hess_lag_vec! of the 9-argument form for 'eq9') or with the
    host hess_lag_vec_ callback; returns (trace, x, obj, ti, operators seen by projcg_, calls made)."""
    P.calls.update(values=0, hlv=0)
    OPT = sys.modules["lfpsqp_jl_amd.optimize"]
    seen, orig = [], OPT.projcg_

    def spy(*args, **kw):
        seen.append((type(args[2]).__name__, getattr(args[2], "fused", None)))
        return orig(*args, **kw)
    par = L.LFPSQPParams(disp=L.DisplayOption.off, **_PAR)
    tr = []
    saved = ctx.options.tridiagonal_one_pass
    ctx.options.tridiagonal_one_pass = one_pass
    OPT.projcg_ = spy
    try:
        if pattern and form == "eq9":
            H = L.SparseLagrangianHessian(P.rows, P.cols, P.values_)
            x, obj, lam, ti = L.optimize(P.f, P.grad_, P.c_, P.jac_c_, H, P.x0, None, None, P.m, par, ctx=ctx, trace=tr)
        else:
            if pattern:
                dv = L.Derivatives(P.grad_, None, P.jac_c_, P.jac_d_, hess_pattern=(P.rows, P.cols), hess_values_=P.values_)
            else:
                dv = L.Derivatives(P.grad_, P.hlv_, P.jac_c_, P.jac_d_)
            x, obj, lam, ti = L.optimize(*P.args("eq" if form == "eq9" else form), par, derivatives=dv, ctx=ctx, trace=tr)
    finally:
        OPT.projcg_ = orig
        ctx.options.tridiagonal_one_pass = saved
    return tr, x, obj, ti, seen, dict(P.calls)


def _check_against_oracle(name, form, tr, x, obj, ti):
    tr0, xr, objr, tir, sens, same = _oracle(name, "eq" if form == "eq9" else form)
    print(f"[sparse pattern {name} {form}] oracle: {tir.iter} iterations, Newton-system iterations {[t.get('tn_iter') for t in tr0]}, "
          f"one-ulp sensitivity {sens:.1e}")
    assert same and sens <= 1e-12                                    # decided on the oracle alone: no exit of its own is borderline
    assert any((t.get('tn_iter') or 0) >= 2 for t in tr0) and any(t.get('steptype') == 1 for t in tr0)
    assert ti.iter == tir.iter and ti.condition.name == tir.condition.name
    assert _compare_traces(tr, tr0, rtol=1e-10) is None
    assert abs(obj[-1] - objr[-1]) <= 1e-11 * abs(objr[-1])
    assert np.linalg.norm(x - xr) <= 1e-10 * np.linalg.norm(xr)


# ---- 6. / 7. trajectory parity, and what crosses PCIe ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("pc567", "eq"), ("pc567", "eq9"), ("pc567", "box"), ("pc567", "slack8"), ("pc567", "slack10"),
                                       ("mesh45", "eq"), ("mesh45", "box")])
def test_pattern_hessian_follows_the_oracle_and_the_callback_run(dev_ctx, name, form):
    ctx = dev_ctx
    P = _problem(name)
    tr, x, obj, ti, seen, calls = _device_run(ctx, P, form, True)
    _check_against_oracle(name, form, tr, x, obj, ti)
    # 7. every Newton solve ran a fused SparseOperator; values_ once per solve at most; the host hess_lag_vec_ never
    solves = sum(1 for t in tr if 'tn_iter' in t)
    assert seen and len(seen) == solves and all(s == ("SparseOperator", True) for s in seen)
    assert 0 < calls["values"] <= solves and calls["hlv"] == 0
    # the same problem through the host callback: the same trajectory, at one round trip per CG iteration
    trc, xc, objc, tic, seenc, callsc = _device_run(ctx, P, form, False)
    assert all(s[0] != "SparseOperator" for s in seenc)
    assert callsc["values"] == 0 and callsc["hlv"] > calls["values"]
    print(f"[sparse pattern {name} {form}] values_ calls {calls['values']} for {solves} solves; host hess_lag_vec_ calls on the callback run "
          f"{callsc['hlv']}")
    assert tic.iter == ti.iter and _compare_traces(tr, trc, rtol=1e-10) is None
    assert np.linalg.norm(x - xc) <= 1e-10 * np.linalg.norm(xc)


# ---- 8. the device callback path, and the row limit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["eq", "box"])
def test_pattern_hessian_on_the_device_callback_path(dev_ctx, form):
    """tridiagonal_one_pass = False: the same SparseOperator with fused off -- lfpsqp_sphess_mul per CG iteration, still no host call inside
    the solve -- and the same trajectory to the same bar."""
    ctx = dev_ctx
    P = _problem("pc567")
    tr, x, obj, ti, seen, calls = _device_run(ctx, P, form, True, one_pass=False)
    _check_against_oracle("pc567", form, tr, x, obj, ti)
    solves = sum(1 for t in tr if 'tn_iter' in t)
    assert seen and all(s == ("SparseOperator", False) for s in seen)
    assert 0 < calls["values"] <= solves and calls["hlv"] == 0


def test_a_row_of_33_neighbours_raises_the_library_error(dev_ctx):
    ctx = dev_ctx
    n = 40
    rows, cols = np.zeros(33, dtype=np.int64), np.arange(1, 34)
    H = L.SparseLagrangianHessian(rows, cols, lambda vals, x, lam: vals.fill(0.0))
    f = lambda x: float(x[:n] @ x[:n])

    def grad_(g, x):
        g[:n] = 2.0 * x[:n]
    with pytest.raises(L.LfpsqpError, match="33 off-diagonal entries"):
        L.optimize(f, np.ones(n), derivatives=L.Derivatives(grad_, None, hess_pattern=(rows, cols), hess_values_=H.values_), ctx=ctx)
    with pytest.raises(ValueError):
        L.optimize(f, np.ones(n), derivatives=L.Derivatives(grad_, None, hess_pattern=(rows, cols)), ctx=ctx)
    with pytest.raises(ValueError):
        L.optimize(f, np.ones(n), derivatives=L.Derivatives(grad_, None, hess_pattern=([0], [n]), hess_values_=H.values_), ctx=ctx)


def test_non_finite_values_raise(dev_ctx):
    ctx = dev_ctx
    P = _problem("pc567")

    def bad(vals, x, lam):
        P._values(vals, x, lam)
        vals[3] = np.nan
    dv = L.Derivatives(P.grad_, None, P.jac_c_, hess_pattern=(P.rows, P.cols), hess_values_=bad)
    with pytest.raises(ValueError, match="non-finite"):
        L.optimize(P.f, P.c_, P.x0, P.m, L.LFPSQPParams(disp=L.DisplayOption.off, **_PAR), derivatives=dv, ctx=ctx)
