"""A parameter per edge and anchors for the pair potentials between points: lfpsqp_sphess_points_values, lfpsqp_anchors_create / _free / _info,
lfpsqp_sphess_pair_eval_ex and the host layers above them (SparseHessian.point_values, PointAnchors, pair_eval(params=, anchors=),
PointPotentialLinear(rest=, anchors=)).

    scale * ( sum_e w_e psi(x_p - x_q; par_e) + sum_k u_k psi(x_{p_k} - a_k; par_k) )

with the kinds, the outputs and the conventions of tests/test_sphess_pair.py, whose graphs, observers (H is read through lfpsqp_sphess_mul over a
distance-2 colouring) and references are imported.

ROUNDING COUNTS, from the expressions of csrc/sphess_pair.hip as written.  A per-edge l_e or delta_e is an exact input, as delta is, and kind 2 forms
1/delta_e^2 on the device as 1.0 / (delta_e delta_e), the two roundings the host spends on it in the uniform call: every count of
tests/test_sphess_pair.py stands -- (count(psi), count(a), CV) = (9, 5, 13) / (11, 6, 15) for kind 1 in 2-D / 3-D, (11, 6, 20) / (12, 6, 21) for kind
2.  An anchor's t_c = fl(x_pc - a_c) is one rounding against the exact difference, like a neighbour's; its (psi, a, b) and v are the neighbour's
expressions; it adds ONE fma to each of the row's chains (g, d, the intra-point sums), after the neighbours.  So with
    D = the largest (neighbours + anchors) of a point
the row sums are bounded as before with deg replaced by D: grad gamma_{D + count(a) + 3}, diag and an entry inside a point gamma_{D + CV + 1}; an entry
between two points is untouched by anchors: gamma_{CV + 2}.  f: an anchor's energy term is fma(2 u, psi, e) -- the doubling is exact, and
eval_finish halves the sum exactly -- so it carries count(psi) like an edge's term, and the sum has at most npoints D terms:
gamma_{npoints D + count(psi) + 1}.  (The issue's "deg + ka" with the two maxima taken separately is at least D: the derivation gives the tighter one.)"""
import ctypes as C
import math
import sys

import numpy as np
import pytest

import lfpsqp_jl_amd as L
from lfpsqp_jl_amd import _capi
from oracle import lfpsqp_ref as R
from oracle import synth

from .helpers import POISON, bits
from .test_capi_retractions import _compare_traces, _note, _sep_host
from .test_projcg_diags import _basis
from .test_projcg_sparse import KAPPA, _solve_stacked_c
from .test_sphess_pair import _BUILDERS, _DEG, _PairNp, _counts, _entries, _dense, _g, _lattice, _mul, _opt_case, _pair_np, _pg
from .test_tridiag_bounds import _stacked_problem


# ---- graphs, parameters, anchors -----------------------------------------------------------------------------------------------------------------
def _small_star(dim, nb):
    """The 20 points of the stars of tests/test_sphess_pair.py with fewer neighbours on the hub 7, so that frozen points fit into its rows."""
    edges = sorted([(min(7, q), max(7, q)) for q in nb] + [(1, 2), (3, 19), (10, 12)])
    base = np.array([[k % 5, k // 5, 0.7 * (k % 3)][:dim] for k in range(20)], dtype=np.float64)
    return 20, edges, base, 1.4


_BUILDERS.setdefault("lat7x9c", (2, lambda: _lattice((7, 9), True)))
_BUILDERS.setdefault("star2s", (2, lambda: _small_star(2, [0, 1, 2, 3, 8, 9, 19])))          # degree 7: 7 + 8 frozen points = 15
_BUILDERS.setdefault("star3s", (3, lambda: _small_star(3, [0, 1, 8, 9, 19])))                # degree 5: 5 + 5 = 10
_BUILDERS.setdefault("star3t", (3, lambda: _small_star(3, [0, 19])))                         # degree 2: 2 + 8 = 10
_DEG.update({"lat7x9c": 8, "star2s": 7, "star3s": 5, "star3t": 2})
_HUB = {"star2": 8, "star3": 8, "star2s": 8, "star3s": 5, "star3t": 8}                      # anchors on the hub (8: LFPSQP_ANCHORS_MAX_POINT)


def _unit(seed, k, dim):
    v = synth.hash_vector(seed, k * dim).reshape(k, dim) + 1e-3
    return v / np.sqrt(np.sum(v * v, axis=1))[:, None]


def _anchors(G, x):
    """(point, pos, u, par): on a star as many as the rows allow on the hub 7, one on the leaf 19 and two on the isolated point 16 (no edge at
    all); on a lattice 0 .. 3 per point, scattered.  par in [0.5, 1.5], the distance to the anchor between 0.5 and 2.5 par, u in [0.5, 1.5]."""
    if G.name.startswith("star"):
        point = np.array([7] * _HUB[G.name] + [19, 16, 16], dtype=np.int64)
        point = point[np.argsort(synth.hash_vector(61, len(point)), kind='stable')]          # (the list in no particular order)
    else:
        cnt = np.minimum((4.0 * np.abs(synth.hash_vector(62, G.npoints))).astype(np.int64), 3)
        point = np.repeat(np.arange(G.npoints, dtype=np.int64), cnt)[::-1].copy()
    k = len(point)
    par = 0.5 + synth.hash_vector(63, k) ** 2
    rho = 1.5 + synth.hash_vector(64, k)
    X = x[:G.nrows].reshape(G.npoints, G.dim)
    pos = X[point] + (par * rho)[:, None] * _unit(65, k, G.dim)
    return point, np.ascontiguousarray(pos), 0.5 + synth.hash_vector(66, k) ** 2, par


def _edge_par(G, x, kind):
    """One parameter per edge: l_e in [0.5, 1.5] with r / l_e inside the range of FINDINGS.md 23 (kind 1), delta_e in [0.5, 2] (kind 2)."""
    ne = len(G.pi)
    if kind == 2:
        return 0.5 + 1.5 * synth.hash_vector(67, ne) ** 2
    X = x[:G.nrows].reshape(G.npoints, G.dim)
    r = np.sqrt(np.sum((X[G.pi] - X[G.pj]) ** 2, axis=1))
    ell = np.clip(r / (1.5 + synth.hash_vector(68, ne)), 0.5, 1.5)
    assert 0.32 <= (r / ell).min() and (r / ell).max() <= 2.97
    return ell


def _shuffled(G, vals):
    """The edge list in another order and half of it mirrored, with its values."""
    o = np.argsort(synth.hash_vector(69, len(G.pi)), kind='stable')
    flip = synth.hash_vector(70, len(G.pi)) > 0
    return np.where(flip, G.pj, G.pi)[o], np.where(flip, G.pi, G.pj)[o], np.asarray(vals, dtype=np.float64)[o]


def _reach(G, point):
    """D of the module docstring and the most anchors on a point."""
    ka = np.bincount(point, minlength=G.npoints)
    deg = np.bincount(np.concatenate([G.pi, G.pj]), minlength=G.npoints)
    return int((deg + ka).max()), int(ka.max())


def _solve(ctx, hh, dg, n, m=6):
    """lfpsqp_projcg_sparse with a materialised basis: its set-up reads the EDGE form of hh, its products the row form."""
    U, _ = _basis(ctx, n, m, False)
    x, lam = ctx.vector(n), ctx.vector(m)
    it, nr = L.projcg_(x, lam, L.SparseOperator(0.0, dg, hh), U, ctx.vector(n, synth.hash_vector(4, n)), None, tol=1e-9, work=L.ProjCGWork(ctx, n, m))
    return it, nr, x.download(), lam.download()


def _same_solve(a, b):
    return a[:2] == b[:2] and np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(bits(a[3]), bits(b[3]))


_CASES = [("lat7x9c", 0), ("lat7x9c", 1), ("lat5x5x3", 0), ("lat5x5x3", 1), ("star2", 1), ("star3", 0)]


# ---- 1. a constant parameter is the uniform call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,extra", _CASES)
def test_a_constant_parameter_is_the_uniform_call_bit_for_bit(dev_ctx, name, extra):
    """P holding l on every edge (given in another order, half of it mirrored), no anchors: f (the full call and the reading kernel), grad, diag,
    H's row form (both triangles read back) and its edge form (lfpsqp_projcg_sparse, whose set-up reads it: x, lambda and counts) have the bits of
    pair_eval(kind, l), for kinds 1 and 2; n is odd for ("lat7x9c", 1), ("lat5x5x3", 0) and ("star2", 1) (the pad row), extra = 1 is a slack row.
    With P = A = NULL the entry is the uniform one for kind 0 too."""
    ctx = dev_ctx
    G = _pg(name)
    n = G.nrows + extra
    w, xh = G.weights(), G.positions(extra)
    W = G.handle(ctx, w, extra)
    x = ctx.vector(n, xh)
    dgh = 3.0 * KAPPA * G.deg + synth.hash_vector(3, n) ** 2

    def run(kind, delta, ex, **kw):
        H = W.like()
        g, d = ctx.vector(n, dgh), ctx.vector(n, dgh)
        if ex:
            fv, f1 = C.c_double(), C.c_double()
            ctx.check(ctx.L.lfpsqp_sphess_pair_eval_ex(ctx.h, W.h, kind, delta, None, None, KAPPA, x.h, C.byref(fv), g.h, d.h, H.h))
            ctx.check(ctx.L.lfpsqp_sphess_pair_eval_ex(ctx.h, W.h, kind, delta, None, None, KAPPA, x.h, C.byref(f1), None, None, None))
            f, f1 = fv.value, f1.value
        else:
            f, f1 = W.pair_eval(kind, delta, KAPPA, x, g, d, H, **kw), W.pair_eval(kind, delta, KAPPA, x, **kw)
        up, lo = _entries(ctx, H, G, n)
        return (f, f1), g.download(), d.download(), up, lo, _solve(ctx, H, d, n)

    def same(a, b):
        return a[0] == b[0] and all(np.array_equal(bits(p), bits(q)) for p, q in zip(a[1:5], b[1:5])) and _same_solve(a[5], b[5])
    for kind in (1, 2):
        P = W.point_values(*_shuffled(G, np.full(len(G.pi), G.delta)))
        assert (P.n, P.nedges, P.row_width, P.edge_width, P.npoints, P.dim) == (W.n, W.nedges, W.row_width, W.edge_width, W.npoints, W.dim)
        ref = run(kind, G.delta, False)
        got = run(kind, -1.0, False, params=P)                       # (delta is not used: its rules do not apply)
        assert same(got, ref) and got[5][0] > 3 and np.isfinite(ref[0][0]) and ref[0][0] > 0.0
        P.close()
    for kind in (0, 1, 2):
        assert same(run(kind, G.delta, True), run(kind, G.delta, False))


# ---- 2. an anchor is an edge to a frozen point -----------------------------------------------------------------------------------------------------
class _Frozen:
    """A graph with one extra point per anchor, appended behind all points in anchor order and joined only to its sensor."""

    def __init__(self, name):
        G = _pg(name)
        self.G = G
        self.x = G.positions()
        self.point, self.pos, self.u, self.par = _anchors(G, self.x)
        na = len(self.point)
        key = name + "+frozen"
        edges = sorted(list(zip(G.pi.tolist(), G.pj.tolist())) + [(int(p), G.npoints + k) for k, p in enumerate(self.point)])
        D, _ = _reach(G, self.point)
        _BUILDERS[key] = (G.dim, lambda: (G.npoints + na, edges, np.concatenate([G.base, self.pos]), G.delta))
        _DEG[key] = D
        self.G2 = _pg(key)
        # per edge of G2: is it an edge of G (then which), or the frozen edge of which anchor
        first = {e: k for k, e in enumerate(zip(G.pi.tolist(), G.pj.tolist()))}
        self.src = np.array([first.get(e, -1) for e in zip(self.G2.pi.tolist(), self.G2.pj.tolist())])
        self.anc = self.G2.pj - G.npoints

    def extend(self, vals, avals):
        return np.where(self.src >= 0, np.asarray(vals)[np.maximum(self.src, 0)], np.asarray(avals)[np.maximum(self.anc, 0)])


_FROZEN = {}


@pytest.mark.parametrize("name,extra", [("star2s", 1), ("star3s", 0), ("star3t", 1), ("lat7x9c", 1), ("lat5x5x3", 0)])
def test_an_anchor_is_an_edge_to_a_frozen_point_bit_for_bit(dev_ctx, name, extra):
    """The same term twice: anchors on G, and a second graph with one extra point per anchor behind all points (x = the anchor's position, edge
    weight u_k, edge parameter par_k).  A row's slots are in increasing index order, so the frozen neighbours of a point come last, in anchor
    order: grad, diag and the entries inside every point of G, and the entries between points of G, have the SAME BITS (kinds 0, 1 and 2; kinds 1
    and 2 with a parameter per edge).  f within the sum of the two counted bounds (the reductions run in another order).
    A point of 3 unknowns has at most 10 neighbours, so the hub of a 3-D star cannot have 5 neighbours AND 8 frozen ones as the 2-D one has 7 and
    8 (row width 31): in 3-D the star of degree 5 carries 5 anchors (row width 32) and a star of degree 2 carries the 8."""
    ctx = dev_ctx
    if name not in _FROZEN:
        _FROZEN[name] = _Frozen(name)
    F = _FROZEN[name]
    G, G2 = F.G, F.G2
    D, ka = _reach(G, F.point)
    assert ka == (_HUB[name] if name.startswith("star") else 3) and G2.deg == D
    n, n2 = G.nrows + extra, G2.nrows + extra
    w = G.weights()
    xh = np.concatenate([F.x, np.full(extra, 7.0)])
    x2h = np.concatenate([F.x, F.pos.ravel(), np.full(extra, 7.0)])
    W, W2 = G.handle(ctx, w, extra), G2.handle(ctx, F.extend(w, F.u), extra)
    assert W2.row_width == G.dim - 1 + G.dim * D
    A = L.PointAnchors(W, F.point, F.pos, F.u, F.par)
    assert (A.nanchors, A.width) == (len(F.point), ka)
    x, x2 = ctx.vector(n, xh), ctx.vector(n2, x2h)
    nx, nx2, ni = len(G.xr), len(G2.xr), len(G.ir)
    dd = G.dim * G.dim
    own = np.repeat(F.src >= 0, dd)                                   # the scalar entries of G2 between points of G, in G's edge order
    assert np.array_equal(F.src[F.src >= 0], np.arange(len(G.pi)))
    for kind in (0, 1, 2):
        par = _edge_par(G, F.x, kind) if kind else None
        P = W.point_values(G.pi, G.pj, par) if kind else None
        P2 = W2.point_values(G2.pi, G2.pj, F.extend(par, F.par)) if kind else None
        H, H2 = W.like(), W2.like()
        g, d, g2, d2 = ctx.vector(n), ctx.vector(n), ctx.vector(n2), ctx.vector(n2)
        f = W.pair_eval(kind, 0.0, KAPPA, x, g, d, H, params=P, anchors=A)
        f2 = W2.pair_eval(kind, 0.0, KAPPA, x2, g2, d2, H2, params=P2)
        assert W.pair_eval(kind, 0.0, KAPPA, x, params=P, anchors=A) == f
        for got, ref in ((g, g2), (d, d2)):
            assert np.array_equal(bits(got.download()[:G.nrows]), bits(ref.download()[:G.nrows]))
        assert np.any(g.download()[:G.nrows] != 0.0) and not np.any(g.download()[G.nrows:])
        up, lo = _entries(ctx, H, G, n)
        up2, lo2 = _entries(ctx, H2, G2, n2)
        for a, b in ((up, up2), (lo, lo2)):
            assert np.array_equal(bits(a[:nx]), bits(b[:nx2][own]))                         # between points of G
            assert np.array_equal(bits(a[nx:]), bits(b[nx2:nx2 + ni]))                      # inside the points of G
        assert kind == 0 or np.count_nonzero(up[nx:]) > 0
        # f: the terms of both sums, in numpy
        T = np.concatenate([(F.x.reshape(G.npoints, G.dim)[G.pi] - F.x.reshape(G.npoints, G.dim)[G.pj]),
                            F.x.reshape(G.npoints, G.dim)[F.point] - F.pos])
        pe = np.concatenate([par, F.par]) if kind else 1.0
        psi = _pair_np(kind, T, pe)[0]
        r = np.sqrt(np.sum(T * T, axis=1))
        mag = float(np.sum(KAPPA * np.concatenate([w, F.u]) * (0.5 * (r + pe) ** 2 if kind == 1 else psi)))
        cpsi = _counts(kind, G.dim)[0] if kind else G.dim + 2
        bf = _g(G.npoints * D + cpsi + 1) + _g(G2.npoints * D + cpsi + 1)
        print(f"[pair eval ex] {name} kind {kind} on {ctx.device_name}: f anchored against frozen {abs(f - f2) / mag / bf:.4f} of {bf:.2e}")
        assert abs(f - f2) <= bf * mag and f > 0.0


# ---- 3. real data against mpmath ---------------------------------------------------------------------------------------------------------------------
_MPX = {}


def _mp_case(name, extra, kind, scale):
    """The definitions in mpmath at 60 digits with t taken exactly from the fp64 inputs; once per case, shared by both devices, read-only:
    (grad, its magnitudes, diag, its magnitudes) per row, (value, magnitude) per stored entry between points and inside a point, (f, magnitude)."""
    key = (name, extra, kind)
    if key not in _MPX:
        import mpmath
        G = _pg(name)
        dim, n = G.dim, G.nrows + extra
        w, x = G.weights(), G.positions(extra)
        point, pos, u, par = _anchors(G, x)
        pe = _edge_par(G, x, kind)
        X = x[:G.nrows].reshape(G.npoints, dim)
        with mpmath.workdps(60):
            mp = mpmath.mpf
            zero = mp(0)

            def pot(t, d):
                q = sum(tc * tc for tc in t)
                if kind == 1:
                    r = mpmath.sqrt(q)
                    return (r - d) ** 2 / 2, (r + d) ** 2 / 2, 1 - d / r, 1 + d / r, d / (r * q)
                s = mpmath.sqrt(1 + q / (d * d))
                return d * d * (s - 1), d * d * (s - 1), 1 / s, 1 / s, -1 / (d * d * s * (1 + q / (d * d)))
            gx, ga, dx, da = ([zero] * n for _ in range(4))
            ix, ia = [zero] * len(G.ir), [zero] * len(G.ir)
            cross, fx, fa = [], zero, zero
            terms = [(p, q_, we, [mp(float(X[p, c])) - mp(float(X[q_, c])) for c in range(dim)], d) for p, q_, we, d in
                     zip(G.pi.tolist(), G.pj.tolist(), w.tolist(), pe.tolist())]
            terms += [(p, -1, uk, [mp(float(X[p, c])) - mp(float(ak[c])) for c in range(dim)], d) for p, ak, uk, d in
                      zip(point.tolist(), pos.tolist(), u.tolist(), par.tolist())]
            for p, q_, we, t, d in terms:
                psi, pmag, a, am, b = pot(t, mp(d))
                sw = mp(scale) * mp(we)
                fx += sw * psi
                fa += sw * pmag
                for c in range(dim):
                    for s_, pt in ((1, p), (-1, q_)):
                        if pt >= 0:
                            gx[dim * pt + c] += s_ * sw * a * t[c]
                            ga[dim * pt + c] += sw * am * abs(t[c])
                            dx[dim * pt + c] += sw * (a + b * t[c] * t[c])
                            da[dim * pt + c] += sw * (am + abs(b) * t[c] * t[c])
                if q_ >= 0:
                    for c, c2 in G.comp.tolist():
                        cross.append((-sw * ((a if c == c2 else zero) + b * t[c] * t[c2]), sw * ((am if c == c2 else zero) + abs(b * t[c] * t[c2]))))
                for k, (c, c2) in enumerate(G.intra.tolist()):
                    for pt in (p, q_):
                        if pt >= 0:
                            ix[pt * len(G.intra) + k] += sw * b * t[c] * t[c2]
                            ia[pt * len(G.intra) + k] += sw * abs(b * t[c] * t[c2])
        _MPX[key] = (gx, ga, dx, da, cross, ix, ia, fx, fa)
    return _MPX[key]


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("name,extra", [("lat7x9c", 1), ("lat5x5x3", 0), ("star2", 0), ("star3", 1)])
def test_real_data_with_parameters_and_anchors_within_the_counted_bounds(dev_ctx, name, extra, kind):
    """Kinds 1 and 2, scale 0.9, w and u in [0.5, 1.5], a parameter per edge (l_e in [0.5, 1.5] with r / l_e inside 0.32 .. 2.97, asserted; delta_e in
    [0.5, 2]) and anchors with their own par_k in [0.5, 1.5] at 0.5 .. 2.5 par_k from their points: 8 on the hub of a star (row width 31 / 32), one
    on a leaf, two on an isolated point; 0 .. 3 per point of a lattice.  Against the definitions at 60 digits, with the counts of the module
    docstring: EVERY row of grad and diag, EVERY stored entry of both triangles, and f (the full call and the reading kernel).
    Observed, as a fraction of the bound -- FINDINGS.md 25 has the table."""
    import mpmath
    ctx = dev_ctx
    G = _pg(name)
    dim, n = G.dim, G.nrows + extra
    w, xh = G.weights(), G.positions(extra)
    point, pos, u, par = _anchors(G, xh)
    D, ka = _reach(G, point)
    gx, ga, dx, da, cross, ix, ia, fx, fa = _mp_case(name, extra, kind, KAPPA)
    cpsi, ca, cv = _counts(kind, dim)
    W = G.handle(ctx, w, extra)
    P = W.point_values(*_shuffled(G, _edge_par(G, xh, kind)))
    A = L.PointAnchors(W, point, pos, u, par)
    assert A.width == ka == (8 if name.startswith("star") else 3)
    H = W.like()
    x, g, d = ctx.vector(n, xh), ctx.vector(n), ctx.vector(n)
    f = W.pair_eval(kind, np.nan, KAPPA, x, g, d, H, params=P, anchors=A)
    f_only = W.pair_eval(kind, np.nan, KAPPA, x, params=P, anchors=A)
    gd, dd = g.download(), d.download()
    up, lo = _entries(ctx, H, G, n)
    nx = len(G.xr)
    assert len(cross) == nx
    with mpmath.workdps(60):
        mp = mpmath.mpf
        live = [i for i in range(n) if ga[i] > 0]
        eg = max(float(abs(mp(float(gd[i])) - gx[i]) / ga[i]) for i in live)
        ed = max(float(abs(mp(float(dd[i])) - dx[i]) / da[i]) for i in live)
        eh = max(float(abs(mp(float(v)) - cross[i][0]) / cross[i][1]) for arr in (up[:nx], lo[:nx]) for i, v in enumerate(arr.tolist()))
        ei = max(float(abs(mp(float(v)) - ix[i]) / ia[i]) for arr in (up[nx:], lo[nx:]) for i, v in enumerate(arr.tolist()) if ia[i] > 0)
        ef = max(float(abs(mp(v) - fx) / fa) for v in (f, f_only))
    bg, bd, bh, bf = _g(D + ca + 3), _g(D + cv + 1), _g(cv + 2), _g(G.npoints * D + cpsi + 1)
    _note(f"pair eval ex {name} kind {kind} dim {dim} D {D} on {ctx.device_name}: grad {eg / bg:.3f} of {bg:.2e}, diag {ed / bd:.3f} of {bd:.2e}, "
          f"inside a point {ei / bd:.3f} of {bd:.2e}, between points {eh / bh:.3f} of {bh:.2e}, f {ef / bf:.4f} of {bf:.2e}")
    assert eg <= bg
    assert ed <= bd
    assert ei <= bd
    assert eh <= bh
    assert ef <= bf
    dead = [i for i in range(n) if ga[i] == 0]
    assert all(gd[i] == 0.0 and dd[i] == 0.0 for i in dead) and len(dead) >= extra
    assert all(v == 0.0 for arr in (up[nx:], lo[nx:]) for i, v in enumerate(arr.tolist()) if ia[i] == 0)
    if name.startswith("star"):                                      # the isolated point 16: two anchors and no edge -- its rows and its own slots live
        assert all(gd[dim * 16 + c] != 0.0 and dd[dim * 16 + c] != 0.0 for c in range(dim))
        k16 = 16 * len(G.intra)
        assert all(v != 0.0 for v in up[nx + k16:nx + k16 + len(G.intra)])


# ---- 4. symmetry and the edge form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,extra,kind", [("lat7x9c", 0, 1), ("lat5x5x3", 1, 2), ("star2", 1, 2), ("star3", 0, 1)])
def test_refreshed_handle_is_symmetric_and_its_edge_form_holds_the_row_form(dev_ctx, name, extra, kind):
    """After a refresh with a parameter per edge and anchors, H read back is bitwise symmetric (both triangles through the colouring; as a dense
    matrix on the lattices), and lfpsqp_projcg_sparse -- its set-up reads the EDGE form, its products the row form -- gives bit-identical x, lambda
    and counts with H and with a handle freshly made by lfpsqp_sphess_create from the values read back (which fills both forms from one value), for a
    materialised basis and for the stacked form under four-way bounds.  Kind 1 is solved next to a diagonal that keeps the matrix positive
    definite."""
    ctx = dev_ctx
    G = _pg(name)
    n, m = G.nrows + extra, 6
    w, xh = G.weights(), G.positions(extra)
    point, pos, u, par = _anchors(G, xh)
    D, _ = _reach(G, point)
    W = G.handle(ctx, w, extra)
    P = W.point_values(G.pi, G.pj, _edge_par(G, xh, kind))
    A = L.PointAnchors(W, point, pos, u, par)
    H = W.like()
    base = 1.0 + 0.5 * synth.hash_vector(3, n) ** 2 + (3.0 * KAPPA * D if kind == 1 else 0.0)
    dg = ctx.vector(n, base)
    W.pair_eval(kind, 0.0, KAPPA, ctx.vector(n, xh), None, dg, H, want_f=False, params=P, anchors=A)
    up, lo = _entries(ctx, H, G, n)
    assert np.array_equal(bits(up), bits(lo)) and np.count_nonzero(up[:len(G.xr)]) == len(G.xr)
    Dm = np.zeros((n, n))
    Dm[G.rows, G.cols] = Dm[G.cols, G.rows] = up
    if name.startswith("lat"):
        Dd = _dense(ctx, H, n)
        assert np.array_equal(bits(Dd), bits(Dd.T)) and np.array_equal(bits(Dd), bits(Dm))
    assert np.linalg.eigvalsh(Dm + np.diag(dg.download()))[0] > 0.01
    S = L.SparseHessian(ctx, n, G.rows, G.cols, up)
    assert (S.row_width, S.edge_width) == (H.row_width, H.edge_width)
    r0, r1 = _solve(ctx, H, dg, n, m), _solve(ctx, S, dg, n, m)
    assert _same_solve(r0, r1) and r0[0] > 3
    Pb, P0, _, rank = _stacked_problem(ctx, n, m, False)
    assert rank == m
    dg2 = L.StackedVector(ctx, n).upload2(np.concatenate([dg.download(), 0.5 + synth.hash_vector(16, n) ** 2]))
    bs = synth.hash_vector(4, 2 * n)
    tmp = np.zeros(n + m)
    R.mul_(tmp, R.adj(P0), bs)
    R.mul_(bs, P0, tmp, -1.0, 1.0)
    b2 = L.StackedVector(ctx, n).upload2(bs)
    res = []
    for hh in (H, S):
        rc, it, nr, xs, lam = _solve_stacked_c(ctx, L.SparseOperator(0.0, dg2, hh), Pb, b2, n, m, 1e-9)
        assert rc == 0 and it > 3
        res.append((it, nr, xs.download2(), lam.download()))
    assert _same_solve(res[0], res[1])


# ---- 5. accumulation and untouched memory --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lat7x9c", "lat5x5x3"])
def test_outputs_accumulate_and_leave_everything_else_alone(dev_ctx, name):
    """Kind 0 with integer data is exact (an anchor is then the pin u |x_p - a|^2 / 2): grad and diag are ADDED to, twice; two trailing rows and the
    y half of a stacked vector keep their bits (POISON); the value-only call writes nothing.  Then kind 1 with a parameter per edge and real
    anchors: W, P and the anchors give the same bits before and after (W and P through a product, the anchors through the value they produce), x is
    unchanged."""
    ctx = dev_ctx
    G = _pg(name)
    nr, n, dim = G.nrows, G.nrows + 2, G.dim
    rng = np.random.default_rng(11)
    w, xi = rng.integers(1, 5, len(G.pi)), rng.integers(-6, 7, nr)
    cnt = np.minimum((4.0 * np.abs(synth.hash_vector(62, G.npoints))).astype(np.int64), 3)
    point = np.repeat(np.arange(G.npoints, dtype=np.int64), cnt)
    ai, ui = rng.integers(-6, 7, (len(point), dim)), rng.integers(1, 5, len(point))
    X = xi.reshape(G.npoints, dim)
    T, Ta = X[G.pi] - X[G.pj], X[point] - ai
    gr = np.zeros((G.npoints, dim), dtype=np.int64)
    np.add.at(gr, G.pi, w[:, None] * T)
    np.add.at(gr, G.pj, -w[:, None] * T)
    np.add.at(gr, point, ui[:, None] * Ta)
    dr = np.zeros(G.npoints, dtype=np.int64)
    np.add.at(dr, G.pi, w)
    np.add.at(dr, G.pj, w)
    np.add.at(dr, point, ui)
    gr, dr = gr.ravel(), np.repeat(dr, dim)
    f2 = int(np.sum(w * np.sum(T * T, axis=1)) + np.sum(ui * np.sum(Ta * Ta, axis=1)))
    W = G.handle(ctx, w.astype(np.float64), 2)
    H = W.like()
    A = L.PointAnchors(W, point, ai.astype(np.float64), ui.astype(np.float64))
    vh = np.random.default_rng(4).integers(-9, 10, n).astype(np.float64)
    w_before, h_before = _mul(ctx, W, vh), _mul(ctx, H, vh)
    xs = np.concatenate([xi, [1e3, 1e3], np.full(n, 1e3)]).astype(np.float64)
    x = L.StackedVector(ctx, n).upload2(xs)
    g0 = np.random.default_rng(5).integers(-50, 51, n).astype(np.float64)
    g0[nr:] = POISON
    g = ctx.vector(n, g0)
    d = L.StackedVector(ctx, n).upload2(np.concatenate([g0, np.full(n, POISON)]))
    d_all = d.download()
    assert W.pair_eval(0, 0.0, 1.0, x, anchors=A) == f2 / 2.0        # value only: nothing written
    assert np.array_equal(bits(_mul(ctx, H, vh)), bits(h_before))
    assert np.array_equal(bits(g.download()), bits(g0)) and np.array_equal(bits(d.download()), bits(d_all))
    assert W.pair_eval(0, 0.0, 1.0, x, grad=g, want_f=False, anchors=A) is None
    assert np.array_equal(g.download()[:nr], g0[:nr] + gr) and np.array_equal(bits(g.download()[nr:]), bits(g0[nr:]))
    assert np.array_equal(bits(d.download()), bits(d_all)) and np.array_equal(bits(_mul(ctx, H, vh)), bits(h_before))
    assert W.pair_eval(0, 0.0, 1.0, x, diag=d, anchors=A) == f2 / 2.0
    assert np.array_equal(d.download()[:nr], g0[:nr] + dr) and np.array_equal(bits(d.download()[nr:]), bits(d_all[nr:]))
    W.pair_eval(0, 0.0, 1.0, x, grad=g, diag=d, out=H, want_f=False, anchors=A)            # a second time: added again
    assert np.array_equal(g.download()[:nr], g0[:nr] + 2 * gr) and np.array_equal(d.download()[:nr], g0[:nr] + 2 * dr)
    assert np.array_equal(bits(g.download()[nr:]), bits(g0[nr:])) and np.array_equal(bits(d.download()[nr:]), bits(d_all[nr:]))
    assert np.any(_mul(ctx, H, vh) != h_before) and np.array_equal(bits(_mul(ctx, W, vh)), bits(w_before))
    ctx.check(ctx.L.lfpsqp_sphess_pair_eval_ex(ctx.h, W.h, 0, 0.0, None, A.h, 1.0, x.h, None, None, None, None))      # nothing asked for
    # kind 1, a parameter per edge, real anchors
    xh = G.positions(2)
    pt, pos, u, par = _anchors(G, xh)
    P = W.point_values(G.pi, G.pj, _edge_par(G, xh, 1))
    A1 = L.PointAnchors(W, pt, pos, u, par)
    xv = ctx.vector(n, xh)
    p_before = _mul(ctx, P, vh)
    f_before = W.pair_eval(1, 0.0, KAPPA, xv, params=P, anchors=A1)
    g1 = ctx.vector(n, g0)
    assert W.pair_eval(1, 0.0, KAPPA, xv, g1, d, H, params=P, anchors=A1) == f_before
    assert np.array_equal(bits(g1.download()[nr:]), bits(g0[nr:])) and np.array_equal(bits(d.download()[nr:]), bits(d_all[nr:]))
    assert np.array_equal(bits(_mul(ctx, P, vh)), bits(p_before)) and np.array_equal(bits(_mul(ctx, W, vh)), bits(w_before))
    assert W.pair_eval(1, 0.0, KAPPA, xv, params=P, anchors=A1) == f_before and np.array_equal(bits(xv.download()), bits(xh))
    assert np.array_equal(bits(x.download2()), bits(xs))


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def _err(ctx):
    return ctx.L.lfpsqp_last_error(ctx.h).decode()


def test_points_values_refuses_what_is_not_exactly_the_edge_list(dev_ctx):
    ctx = dev_ctx
    G = _pg("lat7x9c")
    W = G.handle(ctx, G.weights())
    out = C.c_void_p()
    ne = len(G.pi)

    def call(pi, pj, v, ww=W):
        ii, jj, vv = np.ascontiguousarray(pi, dtype=np.int64), np.ascontiguousarray(pj, dtype=np.int64), np.ascontiguousarray(v, dtype=np.float64)
        rc = ctx.L.lfpsqp_sphess_points_values(ctx.h, ww.h, len(ii), ii.ctypes.data, jj.ctypes.data, vv.ctypes.data, C.byref(out))
        if rc == 0:
            ctx.L.lfpsqp_sphess_free(ctx.h, out)
        else:
            assert out.value is None
        return rc
    one = np.ones(ne)
    assert call(G.pi, G.pj, one) == 0 and call(G.pj, G.pi, 0.0 * one) == 0 and call(G.pi, G.pj, one, W.like()) == 0
    assert call(G.pi[:-1], G.pj[:-1], one[:-1]) == -1 and "1 of the handle's" in _err(ctx) and "missing" in _err(ctx)      # an edge without a value
    far = np.concatenate([G.pi[:-1], [0]]), np.concatenate([G.pj[:-1], [G.npoints - 1]])
    assert call(*far, one) == -1 and f"point edge {ne - 1} is no edge" in _err(ctx)                                        # a foreign edge
    dup = np.concatenate([G.pi[:-1], G.pi[3:4]]), np.concatenate([G.pj[:-1], G.pj[3:4]])
    assert call(*dup, one) == -1 and f"point edge {ne - 1} repeats point edge 3" in _err(ctx)                              # a duplicate
    mir = np.concatenate([G.pi[:-1], G.pj[3:4]]), np.concatenate([G.pj[:-1], G.pi[3:4]])
    assert call(*mir, one) == -1 and f"point edge {ne - 1} repeats point edge 3" in _err(ctx)                              # a mirrored duplicate
    assert call(np.concatenate([G.pi, G.pi[:1]]), np.concatenate([G.pj, G.pj[:1]]), np.ones(ne + 1)) == -1 and "repeats" in _err(ctx)
    for bad in (-0.5, np.nan, np.inf):
        v = one.copy()
        v[5] = bad
        assert call(G.pi, G.pj, v) == -1 and "point edge 5" in _err(ctx)                                                   # negative, NaN
    out_of = G.pi.copy()
    out_of[2] = G.npoints
    assert call(out_of, G.pj, one) == -1 and "point edge 2 out of range" in _err(ctx)
    plain = L.SparseHessian(ctx, G.nrows, G.rows, G.cols, 1.0)
    assert call(G.pi, G.pj, one, plain) == -1                                                                              # not a handle of points
    with pytest.raises(ValueError):
        W.point_values(G.pi, G.pj[:-1], 1.0)


def test_anchors_create_refuses_bad_arguments(dev_ctx):
    ctx = dev_ctx
    G = _pg("lat7x9c")
    W = G.handle(ctx, 1.0)
    out = C.c_void_p()

    def call(point, pos, u, par=None, ww=W):
        pt, ph, uh = np.ascontiguousarray(point, dtype=np.int64), np.ascontiguousarray(pos, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
        rh = None if par is None else np.ascontiguousarray(par, dtype=np.float64)
        rc = ctx.L.lfpsqp_anchors_create(ctx.h, ww.h, len(pt), pt.ctypes.data, ph.ctypes.data, uh.ctypes.data, None if rh is None else rh.ctypes.data,
                                         C.byref(out))
        if rc == 0:
            na, wd = _capi.c_i64(-1), _capi.c_i64(-1)
            assert ctx.L.lfpsqp_anchors_info(out, C.byref(na), C.byref(wd)) == 0 and ctx.L.lfpsqp_anchors_info(out, None, None) == 0
            ctx.L.lfpsqp_anchors_free(ctx.h, out)
            return na.value, wd.value
        assert out.value is None
        return rc
    z = lambda k: np.zeros((k, 2))
    assert call([], z(0), []) == (0, 0) and call([3, 3, 5], z(3), np.ones(3)) == (3, 2) and call([3], z(1), [0.0], [0.0]) == (1, 1)
    assert call([4] * 8, z(8), np.ones(8)) == (8, 8)
    assert call([4] * 9, z(9), np.ones(9)) == -5 and "9 anchors" in _err(ctx) and "> 8" in _err(ctx)                       # the count and the limit
    assert call([G.npoints], z(1), [1.0]) == -1 and "anchor 0" in _err(ctx) and call([0, -1], z(2), [1.0, 1.0]) == -1 and "anchor 1" in _err(ctx)
    for bad in (np.nan, np.inf):
        p = z(2)
        p[1, 1] = bad
        assert call([0, 1], p, [1.0, 1.0]) == -1 and "anchor 1" in _err(ctx) and "not finite" in _err(ctx)
        assert call([0, 1], z(2), [bad, 1.0]) == -1 and "anchor 0" in _err(ctx)
        assert call([0, 1], z(2), [1.0, 1.0], [1.0, bad]) == -1 and "anchor 1" in _err(ctx)
    assert call([0, 1], z(2), [1.0, 1.0], [1.0, -0.5]) == -1 and "anchor 1 is negative" in _err(ctx)
    plain = L.SparseHessian(ctx, G.nrows, G.rows, G.cols, 1.0)
    assert call([0], z(1), [1.0], None, plain) == -1                                                                       # a scalar handle as W
    assert ctx.L.lfpsqp_anchors_info(None, None, None) == -1 and ctx.L.lfpsqp_anchors_free(ctx.h, None) == 0
    with pytest.raises(ValueError):
        L.PointAnchors(W, [0], np.zeros((1, 3)), 1.0)


def _ex_setup(ctx):
    G = _pg("lat7x9c")
    xh = G.positions()
    W = G.handle(ctx, G.weights())
    pt, pos, u, par = _anchors(G, xh)
    return G, W, W.like(), W.point_values(G.pi, G.pj, _edge_par(G, xh, 1)), L.PointAnchors(W, pt, pos, u, par), L.PointAnchors(W, pt, pos, u), \
        ctx.vector(G.nrows, xh), ctx.vector(G.nrows), ctx.vector(G.nrows)


def test_pair_eval_ex_refuses_bad_arguments(dev_ctx):
    ctx = dev_ctx
    G, W, H, P, A, A0, x, g, d = _ex_setup(ctx)
    f = C.c_double()

    def call(kind=1, delta=0.8, pp=P, aa=A, scale=1.0, xx=x, gg=g, dd=d, hh=H, ww=W):
        h = lambda o: None if o is None else o.h
        return ctx.L.lfpsqp_sphess_pair_eval_ex(ctx.h, h(ww), kind, delta, h(pp), h(aa), scale, h(xx), C.byref(f), h(gg), h(dd), h(hh))
    assert call() == 0 and call(kind=2) == 0 and call(aa=None) == 0 and call(pp=None) == 0 and call(pp=None, aa=None) == 0
    other = _pg("lat7x9c").handle(ctx, 1.0)                          # the same points, another pattern object
    Po = other.point_values(G.pi, G.pj, 1.0)
    assert call(pp=Po) == -1 and call(pp=other) == -1                # P on another pattern
    assert call(pp=H, hh=H) == -1 and call(pp=H, hh=None) == 0       # P == H
    assert call(kind=0) == -1 and call(kind=0, pp=None) == 0         # kind 0 has no parameter; anchors are pins
    assert call(kind=-1) == -1 and call(kind=3) == -1
    # delta is checked where it is used: no P, or anchors without par
    for bad in (-0.5, np.nan, np.inf):
        assert call(delta=bad) == 0 and call(kind=2, delta=bad) == 0
        assert call(delta=bad, pp=None) == -1 and call(delta=bad, aa=A0) == -1 and call(kind=2, delta=bad, aa=A0) == -1
        assert call(kind=0, delta=bad, pp=None) == 0
    assert call(kind=2, delta=0.0, pp=None) == -1 and call(kind=2, delta=0.0, aa=A0) == -1 and call(kind=1, delta=0.0, aa=A0) == 0
    # A made for another W
    G3 = _pg("lat5x5x3")
    A3 = L.PointAnchors(G3.handle(ctx, 1.0), [0], np.zeros((1, 3)), 1.0)
    Am = L.PointAnchors(G.handle(ctx, 1.0, 1), [0], np.zeros((1, 2)), 1.0)      # one more row
    assert call(aa=A3) == -1 and call(aa=Am) == -1
    assert call(aa=L.PointAnchors(other, [0], np.zeros((1, 2)), 1.0, 0.5)) == 0      # (the four numbers agree: no reference on its W)
    for bad in (np.nan, np.inf):
        assert call(scale=bad) == -1
    short = ctx.vector(G.nrows - 1)
    assert call(xx=short) == -1 and call(gg=short) == -1 and call(dd=short) == -1 and call(gg=x) == -1 and call(gg=g, dd=g) == -1
    assert call(hh=other) == -1 and call(hh=W) == -1
    plain = L.SparseHessian(ctx, G.nrows, G.rows, G.cols, 1.0)
    assert call(ww=plain, pp=None, hh=None) == -1 and call(ww=None) == -1 and call(xx=None) == -1
    assert call() == 0
    with pytest.raises(L.LfpsqpError):
        W.pair_eval(0, 0.0, 1.0, x, params=P)


def test_pair_eval_ex_refuses_row_shards_and_foreign_objects(emu_lib):
    ctx = L.Context(0, emu_lib)
    ctx2 = L.Context(0, emu_lib)
    try:
        G, W, H, P, A, A0, x, g, d = _ex_setup(ctx)
        W2 = G.handle(ctx2, 1.0)
        with pytest.raises(ValueError):
            W.pair_eval(1, 0.8, 1.0, x, params=W2.like())
        with pytest.raises(ValueError):
            W.pair_eval(1, 0.8, 1.0, x, anchors=L.PointAnchors(W2, [0], np.zeros((1, 2)), 1.0))
        assert W.pair_eval(1, 0.8, 1.0, x, g, d, H, params=P, anchors=A) > 0
        ctx.comm_init_callback(0, 1, lambda ptr, count, op, stream: 0)
        f = C.c_double()
        assert ctx.L.lfpsqp_sphess_pair_eval_ex(ctx.h, W.h, 1, 0.8, P.h, A.h, 1.0, x.h, C.byref(f), g.h, d.h, H.h) == -5
        assert ctx.L.lfpsqp_sphess_pair_eval_ex(ctx.h, W.h, 1, 0.8, None, A.h, 1.0, x.h, C.byref(f), None, None, None) == -5
        assert ctx.L.lfpsqp_sphess_pair_eval_ex(ctx.h, W.h, 1, 0.8, None, None, 1.0, x.h, C.byref(f), None, None, None) == -5
        with pytest.raises(L.LfpsqpError):
            W.pair_eval(1, 0.8, 1.0, x, params=P)
    finally:
        ctx2.close()
        ctx.close()


# ---- 7. PointPotentialLinear with rest lengths and anchors through optimize ---------------------------------------------------------------------------
_ORACLE_RUNS = {}
_PAR = dict(do_project_retract=False, maxiter=8, tn_kappa=1e-6)
_OPT_CASES = [("lat7x9", "ball"), ("lat5x5x3", "box")]


def _truss_case(name, cons):
    """The kind-1 case of tests/test_sphess_pair.py (a lattice stretched to 1.5 delta) with a rest length per edge, delta (1 +- 0.2), and the corner
    points of the lattice anchored at their stretched places with par = 0 (pins) and weight 2."""
    G, n, m, delta, x0, sep_c, a, P0 = _opt_case(name, 1, 1.5, cons)
    rest = delta * (1.0 + 0.2 * synth.hash_vector(71, len(G.pi)))
    place = (1.5 * delta * (G.base - 0.5 * G.base.max(axis=0)))
    corner = np.flatnonzero(np.all((G.base == 0) | (G.base == G.base.max(axis=0)), axis=1)).astype(np.int64)
    assert len(corner) == 2 ** G.dim
    return G, n, m, delta, x0, sep_c, a, P0, rest, (corner, np.ascontiguousarray(place[corner]), np.full(len(corner), 2.0), np.zeros(len(corner)))


class _AnchorNp:
    """kappa sum_k u_k psi(x_p - a_k; par_k), kind 1, in numpy: value, gradient, Hessian product."""

    def __init__(self, G, anchors, scale):
        self.G, (self.pt, self.pos, self.u, self.par), self.scale = G, anchors, scale

    def _t(self, x):
        return x[:self.G.nrows].reshape(self.G.npoints, self.G.dim)[self.pt] - self.pos

    def f(self, x):
        return float(self.scale * np.sum(self.u * _pair_np(1, self._t(x), self.par)[0]))

    def _scatter(self, V):
        out = np.zeros((self.G.npoints, self.G.dim))
        np.add.at(out, self.pt, V)
        return out.ravel()

    def grad(self, x):
        T = self._t(x)
        return self._scatter((self.scale * self.u * _pair_np(1, T, self.par)[1])[:, None] * T)

    def hess_mul(self, x, src):
        T = self._t(x)
        _, a, b = _pair_np(1, T, self.par)
        Dv = src[:self.G.nrows].reshape(self.G.npoints, self.G.dim)[self.pt]
        return self._scatter((self.scale * self.u)[:, None] * (a[:, None] * Dv + (b * np.sum(T * Dv, axis=1))[:, None] * T))


def _oracle_runs(key):
    """The oracle's run and its run from one ulp away; once per case, shared by the emulator and GPU runs, read-only."""
    if key not in _ORACLE_RUNS:
        G, n, m, delta, x0, sep_c, a, P0, rest, anchors = _truss_case(*key)
        phi, d1, d2 = _sep_host(1, a, sep_c)
        pair = _PairNp(G, np.ones(len(G.pi)), 1, rest, KAPPA)
        anc = _AnchorNp(G, anchors, KAPPA)
        ball = P0.R2 is not None
        curv = []

        def f(x):
            return float(np.sum(phi(x[:n]))) + pair.f(x) + anc.f(x)

        def grad_(g, x):
            g[:n] = d1(x[:n]) + pair.grad(x) + anc.grad(x)

        def hlv_(dest, src, x, lam):
            dest[:] = (d2(x) + (2.0 * lam[m] if ball else 0.0)) * src + pair.hess_mul(x, src) + anc.hess_mul(x, src)
            if np.any(src):                                            # (projcg! starts from A 0)
                curv.append(float(src @ dest) / float(src @ src))

        def oracle(xs, trace):
            p = R.LFPSQPParams(disp=R.DisplayOption.off, **_PAR)
            dv0 = P0.derivatives()
            if ball:
                return R.optimize(f, P0.c_, P0.d_, xs, P0.xl, P0.xu, m, 1, p,
                                  derivatives=R.Derivatives(grad_=grad_, hess_lag_vec_=hlv_, jac_c_=dv0.jac_c_, jac_d_=dv0.jac_d_), trace=trace)
            return R.optimize(f, P0.c_, xs, P0.xl, P0.xu, m, p, derivatives=R.Derivatives(grad_=grad_, hess_lag_vec_=hlv_, jac_c_=dv0.jac_c_), trace=trace)
        tr0, tr1 = [], []
        xr, objr, lamr, tir = oracle(x0, tr0)
        c0 = min(curv)
        oracle(np.nextafter(x0, np.inf), tr1)
        sens = [np.linalg.norm(p['x'] - q['x']) / np.linalg.norm(q['x']) for p, q in zip(tr1, tr0)] + [np.inf] * (len(tr0) - len(tr1))
        _ORACLE_RUNS[key] = (tr0, xr, objr, tir, sens, c0)
    return _ORACLE_RUNS[key]


@pytest.mark.parametrize("name,cons", _OPT_CASES)
def test_truss_objective_with_rest_lengths_and_anchors_follows_the_oracle(dev_ctx, name, cons):
    """PointPotentialLinear(pair_kind=1, rest=, anchors=) through `optimize`, in 2-D with the ball and in 3-D with the box, against the oracle
    driven by numpy closures for the same function; structure, spies and the one-ulp sensitivity rule of
    tests/test_sphess_pair.py::test_point_potential_objective_follows_the_oracle.  A lattice stretched to 1.5 of the mean rest length, the rest
    lengths varying by +- 20 %, the corners pinned at their stretched places (par = 0): ON THE ORACLE ALONE the smallest d'Ad / d'd of the run is
    positive (printed; FINDINGS.md 25), so no solve leaves through the negative-curvature branch, which last bits would choose."""
    ctx = dev_ctx
    key = (name, cons)
    G, n, m, delta, x0, sep_c, a, P0, rest, anchors = _truss_case(*key)
    tr0, xr, objr, tir, sens, cmin = _oracle_runs(key)
    _note(f"truss {name} {cons}: oracle alone: smallest d'Ad / d'd {cmin:.3e}; one-ulp sensitivity {max(sens):.1e}")
    assert cmin > 0.0
    ball = P0.R2 is not None
    p = 1 if ball else 0
    kw = dict(R2=P0.R2) if ball else {}
    if "box" in cons:
        kw.update(xl=P0.xl, xu=P0.xu)
    P = L.PointPotentialLinear(ctx, G.npoints, G.dim, m, ctx.matrix(n + p, m + p).hash_fill(1, 0, n, 1.0, n, m), P0.eq.b, 1, a, sep_c,
                               edges=(G.pi, G.pj, 1.0), kappa=KAPPA, pair_kind=1, delta=np.nan, rest=rest, anchors=anchors, **kw)
    S = P.sparse_hessian
    assert (S.n, S.npoints, S.dim) == (n + p, G.npoints, G.dim) and P.params.h != S.h and (P.anchors.nanchors, P.anchors.width) == (2 ** G.dim, 1)
    OPT = sys.modules["lfpsqp_jl_amd.optimize"]
    seen, orig = [], OPT.projcg_
    ex_entry, calls = ctx.L.lfpsqp_sphess_pair_eval_ex, []
    tr = []

    def spy(*args, **kw_):
        seen.append((type(args[2]).__name__, args[2].S is S))
        return orig(*args, **kw_)

    def ex_spy(*args):
        rc = ex_entry(*args)
        calls.append(rc)
        return rc
    OPT.projcg_ = spy
    setattr(ctx.L, "lfpsqp_sphess_pair_eval_ex", ex_spy)
    try:
        x, obj, lam, ti = P.optimize(x0, L.LFPSQPParams(disp=L.DisplayOption.off, **_PAR), trace=tr)
    finally:
        OPT.projcg_ = orig
        setattr(ctx.L, "lfpsqp_sphess_pair_eval_ex", ex_entry)
    assert seen and all(s == ("SparseOperator", True) for s in seen)
    assert len(calls) > len(seen) and all(rc == 0 for rc in calls)
    assert ti.iter == tir.iter and ti.condition.name == tir.condition.name
    assert any((t.get('tn_iter') or 0) >= 2 for t in tr0)
    rtol = max(1e-10, 10.0 * max(sens))
    assert max(sens) <= 1e-12
    assert _compare_traces(tr, tr0, rtol=rtol) is None
    assert abs(obj[-1] - objr[-1]) <= 1e-11 * abs(objr[-1])
    assert np.linalg.norm(x - xr) <= 1e-10 * np.linalg.norm(xr)


# ---- 8. a size at which a workgroup of the vector launches takes several rounds --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", [((188, 189), 2), ((29, 29, 28), 1)])
def test_pair_eval_ex_at_a_size_of_several_rounds(gpu_lib, shape, kind):
    """About 71 000 scalar rows, one row behind the points, a parameter per edge and 2 anchors on every tenth point, as
    tests/test_sphess_pair.py::test_pair_eval_at_a_size_of_several_rounds: a refresh with f, grad and diag against numpy float64 with the kernel's
    expressions, every bound taken TWICE (numpy rounds as often as the device), with D = deg + 2: rows within 2 gamma_{D + count(a) + 3} (grad) and
    2 gamma_{D + CV + 1} (diag); f against math.fsum of numpy's terms within (gamma_{npoints D + count(psi) + 1} + gamma_{count(psi)}) sum |terms|;
    H through one product with a hash vector, rows within 2 gamma_{Kr + D + CV + 1} sum_j |H_ij| |v_j|."""
    ctx = L.Context(0, gpu_lib)
    try:
        npts, edges, base, delta = _lattice(shape)
        dim = len(shape)
        pi, pj = (np.ascontiguousarray(a) for a in np.array(edges, dtype=np.int64).T)
        nr, n, deg = dim * npts, dim * npts + 1, 2 * dim
        D = deg + 2
        assert 70000 <= nr <= 72000
        w = 0.5 + synth.hash_vector(51, len(pi)) ** 2
        xh = np.concatenate([(base + 0.4 * (synth.hash_vector(52, nr).reshape(npts, dim) - 0.5)).ravel(), [7.0]])
        X = xh[:nr].reshape(npts, dim)
        pe = delta * (1.0 + 0.25 * synth.hash_vector(67, len(pi)))
        point = np.repeat(np.arange(0, npts, 10, dtype=np.int64), 2)
        ka = len(point)
        par = delta * (1.0 + 0.25 * synth.hash_vector(63, ka))
        pos = np.ascontiguousarray(X[point] + (par * (1.5 + synth.hash_vector(64, ka)))[:, None] * _unit(65, ka, dim))
        u = 0.5 + synth.hash_vector(66, ka) ** 2
        cpsi, ca, cv = _counts(kind, dim)
        W = L.SparseHessian.from_points(ctx, n, npts, dim, pi, pj, w)
        P = W.point_values(pj, pi, pe)
        A = L.PointAnchors(W, point, pos, u, par)
        assert A.width == 2
        H = W.like()
        kr = W.row_width
        x, g, d = ctx.vector(n, xh), ctx.vector(n), ctx.vector(n)
        f = W.pair_eval(kind, 0.0, KAPPA, x, g, d, H, params=P, anchors=A)
        assert W.pair_eval(kind, 0.0, KAPPA, x, params=P, anchors=A) == f    # (the same reduction from either kernel)
        T, Ta = X[pi] - X[pj], X[point] - pos
        psi, a, b = _pair_np(kind, np.concatenate([T, Ta]), np.concatenate([pe, par]))
        Tt = np.concatenate([T, Ta])
        sw = KAPPA * np.concatenate([w, u])
        r = np.sqrt(np.sum(Tt * Tt, axis=1))
        pall = np.concatenate([pe, par])
        amag, pmag = (1.0 + pall / r, 0.5 * (r + pall) ** 2) if kind == 1 else (a, psi)
        ne = len(pi)
        P1 = np.concatenate([pi, point])

        def scat(V, sign):
            out = np.zeros((npts, dim))
            np.add.at(out, P1, V)
            np.add.at(out, pj, sign * V[:ne])
            return out.ravel()
        eg = np.abs(g.download()[:nr] - scat((sw * a)[:, None] * Tt, -1.0)) / scat((sw * amag)[:, None] * np.abs(Tt), 1.0)
        ed = np.abs(d.download()[:nr] - scat(sw[:, None] * (a[:, None] + b[:, None] * Tt * Tt), 1.0)) / \
            scat(sw[:, None] * (amag[:, None] + np.abs(b)[:, None] * Tt * Tt), 1.0)
        f_np, f_mag = math.fsum((sw * psi).tolist()), math.fsum((sw * pmag).tolist())
        vh = synth.hash_vector(7, n)
        V = vh[:nr].reshape(npts, dim)
        B = sw[:, None, None] * (a[:, None, None] * np.eye(dim)[None] + b[:, None, None] * (Tt[:, :, None] * Tt[:, None, :]))
        Bm = sw[:, None, None] * (amag[:, None, None] * np.eye(dim)[None] + np.abs(b)[:, None, None] * np.abs(Tt[:, :, None] * Tt[:, None, :]))
        off = lambda M: M * (1.0 - np.eye(dim))[None]
        ref = np.zeros((npts, dim))
        mag = np.zeros((npts, dim))
        for P_, Q_ in ((pi, pj), (pj, pi)):
            np.add.at(ref, P_, -np.einsum('eab,eb->ea', B[:ne], V[Q_]) + np.einsum('eab,eb->ea', off(B[:ne]), V[P_]))
            np.add.at(mag, P_, np.einsum('eab,eb->ea', Bm[:ne], np.abs(V[Q_])) + np.einsum('eab,eb->ea', off(Bm[:ne]), np.abs(V[P_])))
        np.add.at(ref, point, np.einsum('eab,eb->ea', off(B[ne:]), V[point]))
        np.add.at(mag, point, np.einsum('eab,eb->ea', off(Bm[ne:]), np.abs(V[point])))
        got = _mul(ctx, H, vh)
        eh = np.abs(got[:nr] - ref.ravel()) / mag.ravel()
        bg, bd, bf, bh = 2 * _g(D + ca + 3), 2 * _g(D + cv + 1), _g(npts * D + cpsi + 1) + _g(cpsi), 2 * _g(kr + D + cv + 1)
        print(f"[pair eval ex {nr}] kind {kind} dim {dim}: grad {eg.max() / bg:.3f} of {bg:.2e}, diag {ed.max() / bd:.3f} of {bd:.2e}, "
              f"f {abs(f - f_np) / f_mag / bf:.4f} of {bf:.2e}, H v {eh.max() / bh:.3f} of {bh:.2e}")
        assert eg.max() <= bg and ed.max() <= bd
        assert abs(f - f_np) <= bf * f_mag
        assert eh.max() <= bh
        assert got[nr] == 0.0 and g.download()[nr] == 0.0 and d.download()[nr] == 0.0
    finally:
        ctx.close()
