"""Pair potentials between points of 2 or 3 unknowns each on the sparse Hessian path: lfpsqp_sphess_create_points, lfpsqp_sphess_points_info,
lfpsqp_sphess_pair_eval and the host layers above them (SparseHessian.from_points / .pair_eval, PointPotentialLinear).

Unknown dim*p + c is component c of point p.  With t = x_p - x_q per undirected point edge and q = |t|^2:  f = scale sum_e w_e psi(t),
grad_(p,c) += scale sum_q w_pq a t_c,  diag_(p,c) += scale sum_q w_pq (a + b t_c^2),  H at ((p,c),(q,c')) = -(scale w_pq)(a [c == c'] + b t_c t_c'),
H at ((p,c),(p,c')) = scale sum_q w_pq b t_c t_c'; kind 0: a = 1, b = 0; kind 1 (a spring of rest length l): psi = (r - l)^2/2, a = 1 - l/r,
b = l/(r q); kind 2 (radial pseudo-Huber): psi = q/(s + 1), a = 1/s, b = -1/(d^2 s (1 + q/d^2)), s = sqrt(1 + q/d^2).  There is no value download
in the ABI: H is observed through lfpsqp_sphess_mul, one indicator vector per colour class of a distance-2 colouring of the SCALAR graph (unit
vectors on the small ones) -- both read entries back exactly, as tests/test_sphess_edge.py does.

ROUNDING COUNTS, from the expressions of csrc/sphess_pair.hip as written, against a reference that takes t = x_p - x_q EXACTLY from the fp64 x
(u = 2^-53; a count k stands for the factor gamma_k; where an expression cancels the bound is on the sum of the magnitudes of its terms):
    t_c = fl(x_pc - x_qc): 1.   q = fma chain over the components: CQ = dim + 2 (t_0 t_0 carries 3; every further fma adds a positive term of
             count 2 and rounds once).
    kind 1:  r = sqrt(q): CR = ceil(CQ/2) + 1 = 3 / 4 (dim 2 / 3).  psi = ((r - l)(r - l))/2 = (r^2 - 2 r l + l^2)/2 with r^2 carrying 2 CR, the
             difference, the square and nothing for the halving: 2 CR + 3 = 9 / 11 on (r + l)^2/2.  a = 1 - l/r: CR + 2 = 5 / 6 on 1 + l/r.
             b = l/(r q): CR + CQ + 2 = 9 / 11.
    kind 2:  1/d^2 = 1/fl(d d) on the host: 2.  u = fma(q, 1/d^2, 1): CQ + 3.  s = sqrt(u): ceil((CQ + 3)/2) + 1 = 5.  psi = q/(s + 1): CQ + 7 =
             11 / 12.  a = 1/s: 6.  b = -(1/d^2)/(s u): 2 + (5 + CQ + 3 + 1) + 1 = CQ + 12 = 16 / 17.
    v = a [c == c'] + b (t_c t_c'), one fma (or one product): t_c t_c' carries 3, so CV = count(b) + 4 = 13 / 15 (kind 1) and 20 / 21 (kind 2), on
             |a|-terms [c == c'] + |b t_c t_c'|, the |a|-terms being 1 + l/r (kind 1) and a (kind 2).
    an entry of H between two points: fl(scale w) and the product: CV + 2.
    a row sum over the deg neighbours of a point (one fma per neighbour, then one rounding with scale): grad, whose term a t_c carries
             count(a) + 2: gamma_{deg + count(a) + 3} sum |a|-terms |t_c|;  diag and an entry of H inside a point: gamma_{deg + CV + 1} sum |terms|.
    f: a term carries count(psi) and then passes, in whatever order lanes, waves, blocks and the second stage take them, through at most
             npoints deg - 1 additions, + 1 for the zero-initialised accumulators, + 1 for the product with scale (halving is exact):
             gamma_{npoints deg + count(psi) + 1} sum |terms|  (the arbitrary-order bound of tests/test_sphess_edge.py).
deg is the largest number of neighbours of a point.  The observed maxima are printed next to each bound, as a fraction of it."""
import ctypes as C
import math
import sys

import numpy as np
import pytest

import lfpsqp_jl_amd as L
from lfpsqp_jl_amd import _capi
from oracle import lfpsqp_ref as R
from oracle import synth

from .helpers import POISON, bits, gamma
from .test_capi_retractions import _compare_traces, _note, _sep_host
from .test_projcg_diags import _basis, _conditioned_tol
from .test_projcg_sparse import KAPPA, _solve_stacked_c
from .test_tridiag_bounds import _stacked_problem


def _g(k):
    return float(gamma(k))


def _counts(kind, dim):
    """(count(psi), count(a), CV) of the module docstring."""
    cq = dim + 2
    if kind == 1:
        cr = (cq + 1) // 2 + 1
        return 2 * cr + 3, cr + 2, cr + cq + 2 + 4
    return cq + 7, 6, cq + 12 + 4


# ---- the point graphs ----------------------------------------------------------------------------------------------------------------------
def _star(dim):
    """20 points: point 7 has the most neighbours a row allows (15 in 2-D: row width 31; 10 in 3-D: 32), lower and higher ones; point 0 has
    higher neighbours only (the slots of its own components come first), point 19 lower ones only (they come last); 15 .. 18 are isolated in
    3-D, 16 .. 18 in 2-D (the slots of their own components are all they have)."""
    nb = list(range(0, 7)) + list(range(8, 15)) + [19] if dim == 2 else list(range(0, 5)) + list(range(8, 12)) + [19]
    edges = sorted([(min(7, q), max(7, q)) for q in nb] + [(1, 2), (3, 19), (10, 12)])
    base = np.array([[k % 5, k // 5, 0.7 * (k % 3)][:dim] for k in range(20)], dtype=np.float64)
    return 20, edges, base, 1.4


def _lattice(shape, corners=False):
    pi, pj = L.grid_edges(shape, corners=corners)
    base = np.indices(shape).reshape(len(shape), -1).T.astype(np.float64)
    return int(np.prod(shape)), sorted(zip(pi.tolist(), pj.tolist())), base, 0.8


# name: (dim, builder); the fourth entry of a builder's result is delta: the rest length of kind 1 and the scale of kind 2
_BUILDERS = {"lat7x9": (2, lambda: _lattice((7, 9))), "lat5x5x3": (3, lambda: _lattice((5, 5, 3))),
             "lat16x20c": (2, lambda: _lattice((16, 20), True)), "lat6x7x8": (3, lambda: _lattice((6, 7, 8))),
             "star2": (2, lambda: _star(2)), "star3": (3, lambda: _star(3))}
_DEG = {"lat7x9": 4, "lat5x5x3": 6, "lat16x20c": 8, "lat6x7x8": 6, "star2": 15, "star3": 10}
_PG = {}


class _PointGraph:
    def __init__(self, name):
        self.name = name
        self.dim, build = _BUILDERS[name]
        self.npoints, edges, self.base, self.delta = build()
        self.pi, self.pj = (np.ascontiguousarray(a) for a in np.array(edges, dtype=np.int64).T)
        assert np.all(self.pi < self.pj) and len(set(edges)) == len(edges)
        d, npts = self.dim, self.npoints
        self.nrows = d * npts
        self.deg = int(np.bincount(np.concatenate([self.pi, self.pj]), minlength=npts).max())
        assert self.deg == _DEG[name]
        # the scalar pattern, rows < cols: per point edge e its dim^2 entries (component pairs in row-major order), then per point its own pairs
        cc = np.array([(a, b) for a in range(d) for b in range(d)])
        self.xr = (d * self.pi[:, None] + cc[None, :, 0]).ravel()
        self.xc = (d * self.pj[:, None] + cc[None, :, 1]).ravel()
        ii = np.array([(a, b) for a in range(d) for b in range(a + 1, d)])
        self.ir = (d * np.arange(npts)[:, None] + ii[None, :, 0]).ravel()
        self.ic = (d * np.arange(npts)[:, None] + ii[None, :, 1]).ravel()
        self.rows, self.cols = np.concatenate([self.xr, self.ir]), np.concatenate([self.xc, self.ic])
        self.comp, self.intra = cc, ii
        # a greedy distance-2 colouring of the scalar graph: no row has two neighbours of one colour
        nb = [[] for _ in range(self.nrows)]
        for a, b in zip(self.rows.tolist(), self.cols.tolist()):
            nb[a].append(b)
            nb[b].append(a)
        col = np.full(self.nrows, -1)
        for v in range(self.nrows):
            used = {col[u] for r in nb[v] for u in nb[r] if u != v}
            k = 0
            while k in used:
                k += 1
            col[v] = k
        self.colour = col
        for a in (self.pi, self.pj, self.rows, self.cols, self.colour, self.base):
            a.setflags(write=False)

    def weights(self):
        return 0.5 + synth.hash_vector(51, len(self.pi)) ** 2

    def positions(self, extra=0, stretch=1.0):
        """The points near their lattice places (spacing `stretch`; hash_vector lies in (-1, 1): every coordinate between 0.6 below and 0.2 above),
        interleaved; `extra` rows behind them hold 7."""
        x = stretch * self.base + 0.4 * (synth.hash_vector(52, self.nrows).reshape(self.npoints, self.dim) - 0.5)
        return np.concatenate([x.ravel(), np.full(extra, 7.0)])

    def handle(self, ctx, w, extra=0):
        return L.SparseHessian.from_points(ctx, self.nrows + extra, self.npoints, self.dim, self.pi, self.pj, w)


def _pg(name):
    if name not in _PG:
        _PG[name] = _PointGraph(name)
    return _PG[name]


# ---- observing H ---------------------------------------------------------------------------------------------------------------------------
def _mul(ctx, S, vh, a0=0.0, dg=None):
    out = ctx.vector(len(vh))
    L.SparseOperator(a0, dg, S).mul_(out, ctx.vector(len(vh), vh))
    return out.download()


def _entries(ctx, S, G, n):
    """(S[rows, cols], S[cols, rows]) for the scalar pattern of G, exactly: one product per colour class."""
    up, lo = np.empty(len(G.rows)), np.empty(len(G.rows))
    ind = np.zeros(n)
    for k in range(G.colour.max() + 1):
        ind[:G.nrows] = G.colour == k
        out = _mul(ctx, S, ind)
        sel = G.colour[G.cols] == k
        up[sel] = out[G.rows[sel]]
        sel = G.colour[G.rows] == k
        lo[sel] = out[G.cols[sel]]
    return up, lo


def _dense(ctx, S, n):
    D = np.empty((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        D[:, j] = _mul(ctx, S, e)
        e[j] = 0.0
    return D


# ---- references ------------------------------------------------------------------------------------------------------------------------------
def _pair_np(kind, T, delta):
    """(psi, a, b) per edge in numpy float64 with the kernel's expressions; T: edges x dim."""
    q = T[:, 0] * T[:, 0]
    for c in range(1, T.shape[1]):
        q = T[:, c] * T[:, c] + q
    if kind == 0:
        return 0.5 * q, np.ones_like(q), np.zeros_like(q)
    if kind == 1:
        r = np.sqrt(q)
        return 0.5 * ((r - delta) * (r - delta)), 1.0 - delta / r, delta / (r * q)
    u = q * (1.0 / (delta * delta)) + 1.0
    s = np.sqrt(u)
    return q / (s + 1.0), 1.0 / s, -((1.0 / (delta * delta)) / (s * u))


class _PairNp:
    """The pair term in numpy over the edge list: value, gradient and Hessian product (the oracle side of PointPotentialLinear) and the entries
    of the Hessian (the large case)."""

    def __init__(self, G, w, kind, delta, scale):
        self.G, self.w, self.kind, self.delta, self.scale = G, np.asarray(w, dtype=np.float64), kind, delta, scale

    def _t(self, x):
        X = x[:self.G.nrows].reshape(self.G.npoints, self.G.dim)
        return X[self.G.pi] - X[self.G.pj]

    def f(self, x):
        return float(self.scale * np.sum(self.w * _pair_np(self.kind, self._t(x), self.delta)[0]))

    def _scatter(self, V):
        G = self.G
        out = np.zeros((G.npoints, G.dim))
        np.add.at(out, G.pi, V)
        np.add.at(out, G.pj, -V)
        return out.ravel()

    def grad(self, x):
        T = self._t(x)
        return self._scatter((self.scale * self.w * _pair_np(self.kind, T, self.delta)[1])[:, None] * T)

    def hess_mul(self, x, src):
        G = self.G
        T = self._t(x)
        _, a, b = _pair_np(self.kind, T, self.delta)
        S = src[:G.nrows].reshape(G.npoints, G.dim)
        D = S[G.pi] - S[G.pj]
        return self._scatter((self.scale * self.w)[:, None] * (a[:, None] * D + (b * np.sum(T * D, axis=1))[:, None] * T))

    def blocks(self, x):
        """scale w (a I + b t t') per edge: edges x dim x dim."""
        T = self._t(x)
        _, a, b = _pair_np(self.kind, T, self.delta)
        return (self.scale * self.w)[:, None, None] * (a[:, None, None] * np.eye(self.G.dim)[None] + b[:, None, None] * (T[:, :, None] * T[:, None, :]))


def _int_case(G, seed):
    """Integer weights 1 .. 4 and integer coordinates in [-6, 6]: |t_c| <= 12, q <= 432, every sum far below 2^53."""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 5, len(G.pi)), rng.integers(-6, 7, G.nrows)


def _int_reference(G, w, x):
    """(2 f, grad, diag) of kind 0 in int64: psi = q/2, a = 1, b = 0."""
    X = x.reshape(G.npoints, G.dim)
    T = X[G.pi] - X[G.pj]
    g = np.zeros((G.npoints, G.dim), dtype=np.int64)
    np.add.at(g, G.pi, w[:, None] * T)
    np.add.at(g, G.pj, -w[:, None] * T)
    deg = np.zeros(G.npoints, dtype=np.int64)
    np.add.at(deg, G.pi, w)
    np.add.at(deg, G.pj, w)
    return int(np.sum(w * np.sum(T * T, axis=1))), g.ravel(), np.repeat(deg, G.dim)


def _created_values(G, vals_cc):
    """The triplet values of a handle with `vals_cc` (one per point edge) on the (c, c) entries of its block and 0.0 on every other entry."""
    blk = np.zeros((len(G.pi), G.dim * G.dim))
    blk[:, ::G.dim + 1] = np.asarray(vals_cc, dtype=np.float64)[:, None]
    return np.concatenate([blk.ravel(), np.zeros(len(G.ir))])


_MP = {}


def _mp_reference(name, kind, scale):
    """The definitions in mpmath at 60 digits, t exactly from the fp64 x; once per case, shared by both devices.  Per edge: scale w psi and its
    magnitude, scale w a and the magnitude of a's terms, scale w b, and t."""
    key = (name, kind)
    if key not in _MP:
        import mpmath
        G = _pg(name)
        w, x = G.weights(), G.positions()
        X = x.reshape(G.npoints, G.dim)
        with mpmath.workdps(60):
            mp = mpmath.mpf
            d = mp(G.delta)
            rows = []
            for p, q_, we in zip(G.pi.tolist(), G.pj.tolist(), w.tolist()):
                t = [mp(float(X[p, c])) - mp(float(X[q_, c])) for c in range(G.dim)]
                q = sum(tc * tc for tc in t)
                if kind == 1:
                    r = mpmath.sqrt(q)
                    psi, pmag, a, amag, b = (r - d) ** 2 / 2, (r + d) ** 2 / 2, 1 - d / r, 1 + d / r, d / (r * q)
                else:
                    s = mpmath.sqrt(1 + q / (d * d))
                    psi, a, b = d * d * (s - 1), 1 / s, -1 / (d * d * s * (1 + q / (d * d)))
                    pmag, amag = psi, a
                sw = mp(scale) * mp(we)
                rows.append((sw * psi, sw * pmag, sw * a, sw * amag, sw * b, t))
            _MP[key] = rows
    return _MP[key]


# ---- 1. kind 0 is exact ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("name", ["lat7x9", "lat5x5x3", "star2", "star3"])
def test_kind_0_with_integer_data_is_exact(dev_ctx, name, extra):
    """f, grad and diag `==` the int64 reference, and H has the bits of a handle made by lfpsqp_sphess_create from -scale w on the (c, c) entries
    and 0.0 on every other entry of the pattern (products with an integer vector and with a hash vector next to a diagonal)."""
    ctx = dev_ctx
    G = _pg(name)
    w, xi = _int_case(G, 7)
    f2, gr, dr = _int_reference(G, w, xi)
    n = G.nrows + extra
    W = G.handle(ctx, w.astype(np.float64), extra)
    assert (W.n, W.npoints, W.dim, W.nedges) == (n, G.npoints, G.dim, len(G.rows))
    assert W.row_width == G.dim - 1 + G.dim * G.deg
    H = W.like()
    xh = np.concatenate([xi.astype(np.float64), np.full(extra, 7.0)])
    x, g, d = ctx.vector(n, xh), ctx.vector(n), ctx.vector(n)
    scale = 2.0
    f = W.pair_eval(0, 0.0, scale, x, g, d, H)
    assert f == float(f2) and W.pair_eval(0, 0.0, scale, x) == float(f2)              # (scale f = 2 sum w q / 2; the full call and the reading kernel)
    assert np.array_equal(g.download()[:G.nrows], scale * gr) and np.array_equal(d.download()[:G.nrows], scale * dr)
    assert not np.any(g.download()[G.nrows:]) and not np.any(d.download()[G.nrows:])
    S = L.SparseHessian(ctx, n, G.rows, G.cols, _created_values(G, -(scale * w)))
    assert (S.row_width, S.edge_width) == (W.row_width, W.edge_width)
    up, lo = _entries(ctx, H, G, n)
    want = _created_values(G, -(scale * w))
    assert np.array_equal(bits(up), bits(want)) and np.array_equal(bits(lo), bits(want))
    vi = np.random.default_rng(3).integers(-9, 10, n).astype(np.float64)
    assert np.array_equal(bits(_mul(ctx, H, vi)), bits(_mul(ctx, S, vi)))
    vh = synth.hash_vector(7, n)
    dg = ctx.vector(n, 1.0 + synth.hash_vector(3, n))
    got, ref = _mul(ctx, H, vh, 0.25, dg), _mul(ctx, S, vh, 0.25, dg)
    assert np.array_equal(bits(got), bits(ref)) and np.any(got[:G.nrows] != ((1.25 + synth.hash_vector(3, n)) * vh)[:G.nrows])


# ---- 2. kinds 1 and 2 against mpmath -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("name", ["lat16x20c", "lat6x7x8", "star2", "star3"])
def test_real_data_within_the_counted_bounds(dev_ctx, name, kind):
    """Kinds 1 and 2, scale = 0.9, w in [0.5, 1.5], every coordinate between 0.6 below and 0.2 above its lattice place (delta = 0.8 on the lattices, 1.4 on the
    stars: r / l between 0.3 and 3, asserted; 0.32 .. 2.97 as it is), against the definitions at 60 digits; the counts are those of the module docstring.  With
    deg the largest number of neighbours:  grad within gamma_{deg + count(a) + 3} sum |a|-terms |t_c|,  diag and the entries inside a point within
    gamma_{deg + CV + 1} sum |terms|,  the entries between points within gamma_{CV + 2} (|a|-terms [c == c'] + |b t_c t_c'|),  f within
    gamma_{npoints deg + count(psi) + 1} sum |terms|;  (count(psi), count(a), CV) = (9, 5, 13) / (11, 6, 15) for kind 1 in 2-D / 3-D and
    (11, 6, 20) / (12, 6, 21) for kind 2.
    Observed, as a fraction of the bound (grad, diag, inside a point, between points, f) -- FINDINGS.md 23 has the table for both devices."""
    import mpmath
    ctx = dev_ctx
    G = _pg(name)
    dim, npts, deg = G.dim, G.npoints, G.deg
    w, xh = G.weights(), G.positions()
    ref = _mp_reference(name, kind, KAPPA)
    cpsi, ca, cv = _counts(kind, dim)
    n = G.nrows
    W = G.handle(ctx, w)
    H = W.like()
    x, g, d = ctx.vector(n, xh), ctx.vector(n), ctx.vector(n)
    f = W.pair_eval(kind, G.delta, KAPPA, x, g, d, H)
    f_only = W.pair_eval(kind, G.delta, KAPPA, x)
    gd, dd = g.download(), d.download()
    up, lo = _entries(ctx, H, G, n)
    nx = len(G.xr)
    with mpmath.workdps(60):
        mp = mpmath.mpf
        zero = mp(0)
        rr = [math.sqrt(float(sum(tc * tc for tc in r[5]))) / G.delta for r in ref]
        assert 0.3 <= min(rr) and max(rr) <= 3.0
        gx, ga, dx, da = ([zero] * n for _ in range(4))
        ix, ia = [zero] * len(G.ir), [zero] * len(G.ir)
        eh = 0.0
        for e, ((_, _, a, am, b, t), p, q) in enumerate(zip(ref, G.pi.tolist(), G.pj.tolist())):
            for c in range(dim):
                for s_, pt in ((1, p), (-1, q)):
                    gx[dim * pt + c] += s_ * a * t[c]
                    ga[dim * pt + c] += am * abs(t[c])
                    dx[dim * pt + c] += a + b * t[c] * t[c]
                    da[dim * pt + c] += am + abs(b) * t[c] * t[c]
            for k, (c, c2) in enumerate(G.comp.tolist()):
                val = -((a if c == c2 else zero) + b * t[c] * t[c2])
                mag = (am if c == c2 else zero) + abs(b * t[c] * t[c2])
                for got in (up[e * dim * dim + k], lo[e * dim * dim + k]):
                    eh = max(eh, float(abs(mp(float(got)) - val) / mag))
            for k, (c, c2) in enumerate(G.intra.tolist()):
                for pt in (p, q):
                    ix[pt * len(G.intra) + k] += b * t[c] * t[c2]
                    ia[pt * len(G.intra) + k] += abs(b * t[c] * t[c2])
        eg = max(float(abs(mp(float(gd[i])) - gx[i]) / ga[i]) for i in range(n) if ga[i] > 0)
        ed = max(float(abs(mp(float(dd[i])) - dx[i]) / da[i]) for i in range(n) if da[i] > 0)
        ei = max(float(abs(mp(float(v)) - ix[i]) / ia[i]) for arr in (up[nx:], lo[nx:]) for i, v in enumerate(arr.tolist()) if ia[i] > 0)
        fx, fa = mpmath.fsum(r[0] for r in ref), mpmath.fsum(r[1] for r in ref)
        ef = max(float(abs(mp(v) - fx) / fa) for v in (f, f_only))
    bg, bd, bh, bf = _g(deg + ca + 3), _g(deg + cv + 1), _g(cv + 2), _g(npts * deg + cpsi + 1)
    print(f"[pair eval] {name} kind {kind} dim {dim} deg {deg} on {ctx.device_name}: grad {eg / bg:.3f} of {bg:.2e}, diag {ed / bd:.3f} of {bd:.2e}, "
          f"inside a point {ei / bd:.3f} of {bd:.2e}, between points {eh / bh:.3f} of {bh:.2e}, f {ef / bf:.4f} of {bf:.2e}")
    assert eg <= bg
    assert ed <= bd
    assert ei <= bd
    assert eh <= bh
    assert ef <= bf
    iso = [i for i in range(n) if ga[i] == 0]
    assert all(gd[i] == 0.0 and dd[i] == 0.0 for i in iso) and (len(iso) > 0) == name.startswith("star")
    assert all(v == 0.0 for arr in (up[nx:], lo[nx:]) for i, v in enumerate(arr.tolist()) if ia[i] == 0)     # an isolated point: its slots hold 0


# ---- 3. symmetry and the edge form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,extra,kinds", [("lat7x9", 0, (1, 2)), ("lat5x5x3", 1, (1, 2)), ("star2", 1, (2,)), ("star3", 0, (2,))])
def test_refreshed_handle_is_symmetric_and_its_edge_form_holds_the_row_form(dev_ctx, name, extra, kinds):
    """After a refresh H read back is bitwise symmetric (both triangles through the colouring; as a dense matrix on the lattices).  Then
    lfpsqp_projcg_sparse -- its set-up reads the EDGE form, its products the row form -- runs with the refreshed H and with a handle freshly made by
    lfpsqp_sphess_create from the values read back (which fills both forms from one value): bit-identical x, lambda and counts, for a materialised
    basis and for the stacked form under four-way bounds.  The materialised solve is also the oracle's projcg! with the dense matrix: its count
    with iterates within 1e-10, under the exit-condition rule and the 1.1 margins of tests/test_projcg_sparse.py, asserted on the oracle first.
    Kind 2 is convex; kind 1 is solved next to a diagonal that keeps the matrix positive definite.  On the stars (40 and 60 unknowns, isolated
    points) the diagonal starts from 1 instead of 0.05: with 0.05 the oracle alone needs 55 iterations in a space of dimension 54."""
    ctx = dev_ctx
    G = _pg(name)
    n, m = G.nrows + extra, 6
    w, xh = G.weights(), G.positions(extra)
    W = G.handle(ctx, w, extra)
    for kind in kinds:
        H = W.like()
        base = (0.05 if name.startswith("lat") else 1.0) + 0.5 * synth.hash_vector(3, n) ** 2
        if kind == 1:
            base += 2.0 * KAPPA * G.deg
        dg = ctx.vector(n, base)
        W.pair_eval(kind, G.delta, KAPPA, ctx.vector(n, xh), None, dg, H, want_f=False)
        up, lo = _entries(ctx, H, G, n)
        assert np.array_equal(bits(up), bits(lo))
        blk = _PairNp(G, w, kind, G.delta, KAPPA).blocks(xh)
        nx = len(G.xr)
        assert np.abs(up[:nx] + blk.reshape(-1)).max() <= 1e-13 and np.count_nonzero(up[:nx]) == nx      # (every slot was written; no stale weight)
        D = np.zeros((n, n))
        D[G.rows, G.cols] = D[G.cols, G.rows] = up
        if name.startswith("lat"):
            Dd = _dense(ctx, H, n)
            assert np.array_equal(bits(Dd), bits(Dd.T)) and np.array_equal(bits(Dd), bits(D))
        S = L.SparseHessian(ctx, n, G.rows, G.cols, up)
        assert (S.row_width, S.edge_width) == (H.row_width, H.edge_width)
        Aref = D + np.diag(dg.download())
        assert np.linalg.eigvalsh(Aref)[0] > 0.01
        # a materialised basis
        U, Uh = _basis(ctx, n, m, False)
        bh = synth.hash_vector(4, n)
        tol, i_base, mu, md = _conditioned_tol(Aref, Uh, bh, np.zeros(m), m)
        print(f"[pair eval] refreshed {name} kind {kind}: oracle {i_base} iterations at 1e-10, tol {tol:.3e}, margins {mu:.2f} / {md:.2f}")
        assert mu >= 1.1 and md >= 1.1
        assert i_base < n - m                                        # (in exact arithmetic CG ends by then: a count that reaches it is made of rounding)
        x0, l0 = np.zeros(n), np.zeros(m)
        i0, nr0 = R.projcg_(x0, l0, Aref, Uh, bh, np.zeros(m), tol=tol)
        res = []
        for hh in (H, S):
            x, lam = ctx.vector(n), ctx.vector(m)
            it, nr = L.projcg_(x, lam, L.SparseOperator(0.0, dg, hh), U, ctx.vector(n, bh), None, tol=tol, work=L.ProjCGWork(ctx, n, m))
            res.append((it, nr, x.download(), lam.download()))
        assert res[0][:2] == res[1][:2] and np.array_equal(bits(res[0][2]), bits(res[1][2])) and np.array_equal(bits(res[0][3]), bits(res[1][3]))
        i1, nr1, xd, ld = res[0]
        dx, dl = np.linalg.norm(xd - x0) / np.linalg.norm(x0), np.abs(ld - l0).max()
        print(f"[pair eval]   iterations {i1} (oracle {i0}), nr {nr1:.6e} ({nr0:.6e}), x {dx:.1e}, lambda {dl:.1e}")
        assert i1 == i0 == i_base and i1 > 3 and nr1 == pytest.approx(nr0, rel=1e-5)
        assert dx <= 1e-10 and dl <= 1e-10
        # the stacked form under bounds
        P, P0, _, rank = _stacked_problem(ctx, n, m, False)
        assert rank == m
        dg2 = L.StackedVector(ctx, n).upload2(np.concatenate([dg.download(), 0.5 + synth.hash_vector(16, n) ** 2]))
        bs = synth.hash_vector(4, 2 * n)
        tmp = np.zeros(n + m)
        R.mul_(tmp, R.adj(P0), bs)
        R.mul_(bs, P0, tmp, -1.0, 1.0)
        b2 = L.StackedVector(ctx, n).upload2(bs)
        res = []
        for hh in (H, S):
            rc, it, nr, x, lam = _solve_stacked_c(ctx, L.SparseOperator(0.0, dg2, hh), P, b2, n, m, 1e-9)
            assert rc == 0 and it > 3
            res.append((it, nr, x.download2(), lam.download()))
        assert res[0][:2] == res[1][:2] and np.array_equal(bits(res[0][2]), bits(res[1][2])) and np.array_equal(bits(res[0][3]), bits(res[1][3]))


# ---- 4. accumulation and untouched memory ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lat7x9", "lat5x5x3"])
def test_outputs_accumulate_and_leave_everything_else_alone(dev_ctx, name):
    """grad and diag are added to; entries >= dim*npoints (two trailing rows, the gap and the y half of a stacked vector) keep their bits; a
    stacked x is read on its x half; every output may be NULL on its own; the value-only call writes nothing; W is never modified."""
    ctx = dev_ctx
    G = _pg(name)
    nr, n = G.nrows, G.nrows + 2
    w, xi = _int_case(G, 11)
    f2, gr, dr = _int_reference(G, w, xi)
    W = G.handle(ctx, w.astype(np.float64), 2)
    H = W.like()
    vh = np.random.default_rng(4).integers(-9, 10, n).astype(np.float64)
    w_before, h_before = _mul(ctx, W, vh), _mul(ctx, H, vh)
    assert np.array_equal(bits(w_before), bits(h_before))            # (like: initialised to W's values)
    x = L.StackedVector(ctx, n).upload2(np.concatenate([xi, [1e3, 1e3], np.full(n, 1e3)]).astype(np.float64))
    g0 = np.random.default_rng(5).integers(-50, 51, n).astype(np.float64)
    g0[nr:] = POISON
    g = ctx.vector(n, g0)
    d = L.StackedVector(ctx, n).upload2(np.concatenate([g0, np.full(n, POISON)]))
    d_all = d.download()
    assert W.pair_eval(0, 0.0, 1.0, x) == f2 / 2.0                   # value only: nothing written
    assert np.array_equal(bits(_mul(ctx, H, vh)), bits(h_before))
    assert np.array_equal(bits(g.download()), bits(g0)) and np.array_equal(bits(d.download()), bits(d_all))
    assert W.pair_eval(0, 0.0, 1.0, x, grad=g, want_f=False) is None
    assert np.array_equal(g.download()[:nr], g0[:nr] + gr) and np.array_equal(bits(g.download()[nr:]), bits(g0[nr:]))
    assert np.array_equal(bits(d.download()), bits(d_all)) and np.array_equal(bits(_mul(ctx, H, vh)), bits(h_before))
    assert W.pair_eval(0, 0.0, 1.0, x, diag=d) == f2 / 2.0
    got = d.download()
    assert np.array_equal(got[:nr], g0[:nr] + dr) and np.array_equal(bits(got[nr:]), bits(d_all[nr:]))
    assert np.array_equal(bits(_mul(ctx, H, vh)), bits(h_before))
    W.pair_eval(0, 0.0, 1.0, x, grad=g, diag=d, out=H, want_f=False)                       # a second time: added again
    assert np.array_equal(g.download()[:nr], g0[:nr] + 2 * gr) and np.array_equal(d.download()[:nr], g0[:nr] + 2 * dr)
    assert np.array_equal(bits(g.download()[nr:]), bits(g0[nr:])) and np.array_equal(bits(d.download()[nr:]), bits(d_all[nr:]))
    S = L.SparseHessian(ctx, n, G.rows, G.cols, _created_values(G, -w.astype(np.float64)))
    assert np.array_equal(bits(_mul(ctx, H, vh)), bits(_mul(ctx, S, vh))) and np.any(_mul(ctx, H, vh) != h_before)
    assert W.pair_eval(0, 0.0, 1.0, x, out=H, want_f=False) is None
    ctx.check(ctx.L.lfpsqp_sphess_pair_eval(ctx.h, W.h, 0, 0.0, 1.0, x.h, None, None, None, None))      # nothing asked for
    assert np.array_equal(bits(_mul(ctx, W, vh)), bits(w_before))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_create_points_refuses_bad_arguments(dev_ctx):
    ctx = dev_ctx
    out = C.c_void_p()

    def create(n, npoints, dim, pi, pj, w):
        ii, jj, ww = np.asarray(pi, dtype=np.int64), np.asarray(pj, dtype=np.int64), np.asarray(w, dtype=np.float64)
        rc = ctx.L.lfpsqp_sphess_create_points(ctx.h, n, npoints, dim, len(ii), ii.ctypes.data, jj.ctypes.data, ww.ctypes.data, C.byref(out))
        if rc == 0:
            ctx.L.lfpsqp_sphess_free(ctx.h, out)
        else:
            assert out.value is None
        return rc
    assert create(8, 4, 2, [0, 1], [1, 2], [1.0, 2.0]) == 0 and create(13, 4, 3, [0, 1], [1, 2], [1.0, 2.0]) == 0
    assert create(4, 4, 1, [0], [1], [1.0]) == -1 and create(16, 4, 4, [0], [1], [1.0]) == -1            # dim
    assert create(7, 4, 2, [0], [1], [1.0]) == -1 and create(11, 4, 3, [0], [1], [1.0]) == -1            # n < dim npoints
    assert create(8, 4, 2, [1], [1], [1.0]) == -1                                                          # p == q
    assert create(8, 4, 2, [0], [4], [1.0]) == -1 and create(8, 4, 2, [-1], [2], [1.0]) == -1            # out of range
    for bad in (np.nan, np.inf, -np.inf):
        assert create(8, 4, 2, [0], [1], [bad]) == -1
    for dim, most in ((2, 15), (3, 10)):
        hub = np.zeros(most + 1, dtype=np.int64)
        assert create(dim * (most + 2), most + 2, dim, hub[:most], np.arange(1, most + 1), np.ones(most)) == 0
        assert create(dim * (most + 2), most + 2, dim, hub, np.arange(1, most + 2), np.ones(most + 1)) == -5
        msg = ctx.L.lfpsqp_last_error(ctx.h).decode()
        assert f"{most + 1} neighbours" in msg and f"> {most} " in msg          # (the point's degree and the limit for this dim)
        # (a duplicate, mirrored, is no further neighbour)
        assert create(dim * (most + 2), most + 2, dim, np.concatenate([hub[:most], [1]]), np.concatenate([np.arange(1, most + 1), [0]]), np.ones(most + 1)) == 0
    with pytest.raises(ValueError):
        L.SparseHessian.from_points(ctx, 8, 4, 2, [0, 1], [1], 1.0)


def _refusal_setup(ctx):
    G = _pg("lat7x9")
    w, xh = G.weights(), G.positions()
    W = G.handle(ctx, w)
    return G.nrows, W, W.like(), G.handle(ctx, w), L.SparseHessian(ctx, G.nrows, G.rows, G.cols, 1.0), ctx.vector(G.nrows, xh), ctx.vector(G.nrows), \
        ctx.vector(G.nrows)


def test_pair_eval_refuses_bad_arguments(dev_ctx):
    ctx = dev_ctx
    n, W, H, other, plain, x, g, d = _refusal_setup(ctx)
    f = C.c_double()

    def call(kind=2, delta=0.8, scale=1.0, xx=x, gg=g, dd=d, hh=H, ww=W):
        h = lambda o: None if o is None else o.h
        return ctx.L.lfpsqp_sphess_pair_eval(ctx.h, h(ww), kind, delta, scale, h(xx), C.byref(f), h(gg), h(dd), h(hh))
    assert call() == 0
    assert call(kind=-1) == -1 and call(kind=3) == -1
    for bad in (0.0, -0.5, np.nan, np.inf):
        assert call(delta=bad) == -1                                 # kind 2: delta > 0
        assert call(kind=0, delta=bad) == 0                          # (kind 0 ignores delta)
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        assert call(kind=1, delta=bad) == -1                         # kind 1: delta >= 0
    assert call(kind=1, delta=0.0) == 0
    for bad in (np.nan, np.inf, -np.inf):
        assert call(scale=bad) == -1
    short = ctx.vector(n - 1)
    assert call(xx=short) == -1 and call(gg=short) == -1 and call(dd=short) == -1
    assert call(gg=x) == -1 and call(dd=x) == -1 and call(gg=g, dd=g) == -1              # aliasing
    assert call(hh=other) == -1                                      # the same points, another pattern object
    assert call(hh=W) == -1                                          # H == W: the weights would be lost
    assert call(ww=plain, hh=None) == -1 and call(ww=plain.like(), hh=None) == -1        # not a handle of points
    assert call(ww=None) == -1 and call(xx=None) == -1
    assert call(xx=L.StackedVector(ctx, n), gg=None, dd=None) == 0   # a longer x is fine
    assert call(hh=None) == 0 and call(ww=H, hh=W) == 0 and call() == 0                  # (a handle on the pattern of points is one of points)


def test_pair_eval_refuses_row_shards_and_foreign_handles(emu_lib):
    ctx = L.Context(0, emu_lib)
    ctx2 = L.Context(0, emu_lib)
    try:
        n, W, H, other, plain, x, g, d = _refusal_setup(ctx)
        G = _pg("lat7x9")
        H2 = G.handle(ctx2, 1.0)
        with pytest.raises(ValueError):
            W.pair_eval(2, 0.8, 1.0, x, out=H2)
        H2.close()
        assert W.pair_eval(2, 0.8, 1.0, x, g, d, H) > 0
        ctx.comm_init_callback(0, 1, lambda ptr, count, op, stream: 0)
        f = C.c_double()
        assert ctx.L.lfpsqp_sphess_pair_eval(ctx.h, W.h, 2, 0.8, 1.0, x.h, C.byref(f), g.h, d.h, H.h) == -5
        assert ctx.L.lfpsqp_sphess_pair_eval(ctx.h, W.h, 2, 0.8, 1.0, x.h, C.byref(f), None, None, None) == -5
        with pytest.raises(L.LfpsqpError):
            W.pair_eval(2, 0.8, 1.0, x)
    finally:
        ctx2.close()
        ctx.close()


# ---- 6. points_info ------------------------------------------------------------------------------------------------------------------------------
def test_points_info_on_both_kinds_of_handle(dev_ctx):
    ctx = dev_ctx
    G = _pg("lat5x5x3")
    W = G.handle(ctx, 1.0, 1)
    plain = L.SparseHessian(ctx, G.nrows, G.rows, G.cols, 1.0)
    npts, dim = _capi.c_i64(-1), _capi.c_i64(-1)
    for S, want in ((W, (75, 3)), (W.like(), (75, 3)), (W.like().like(), (75, 3)), (plain, (0, 0)), (plain.like(), (0, 0)), (_pg("lat7x9").handle(ctx, 2.0), (63, 2))):
        assert ctx.L.lfpsqp_sphess_points_info(S.h, C.byref(npts), C.byref(dim)) == 0 and (npts.value, dim.value) == want
        assert (S.npoints, S.dim) == want
        assert ctx.L.lfpsqp_sphess_points_info(S.h, None, None) == 0
    assert ctx.L.lfpsqp_sphess_points_info(None, C.byref(npts), C.byref(dim)) == -1
    assert (W.n, W.nedges, W.row_width) == (226, 9 * len(G.pi) + 3 * 75, 2 + 3 * 6)


# ---- 7. PointPotentialLinear through optimize ----------------------------------------------------------------------------------------------------
_ORACLE_RUNS = {}
_PAR = dict(do_project_retract=False, maxiter=8, tn_kappa=1e-6)
# (graph, pair kind, the lattice spacing in units of delta, the constraint set)
_OPT_CASES = [("lat7x9", 2, 1.0, "ball+box"), ("lat5x5x3", 2, 1.0, "box"), ("lat7x9", 1, 1.5, "ball")]


def _opt_case(name, pair_kind, spacing, cons):
    """Everything both sides share: the points start near a lattice of spacing `spacing` delta inside (-0.95, 0.95)^dim, the separable term
    a (t^4 + t^2)-type anchor at 1.15 times those places (beyond the box and the ball), the equalities pass through a jittered copy of the start."""
    G = _pg(name)
    n, m = G.nrows, 4
    extent = (G.base.max(axis=0)).max()
    delta = 1.8 / (spacing * extent)
    place = (spacing * delta * (G.base - 0.5 * G.base.max(axis=0))).ravel()
    x0 = place + 0.1 * delta * (synth.hash_vector(2, n) - 0.5)
    anchor = 1.15 * place + 0.05 * delta * (synth.hash_vector(22, n) - 0.5)
    a = 0.5 + synth.hash_vector(21, n) ** 2
    Jh = synth.hash_matrix(1, n, m)
    P0 = synth.BallBoxProblem(n, m, b=Jh.T @ (place + 0.1 * delta * (synth.hash_vector(23, n) - 0.5)))
    if "box" not in cons:
        P0.xl, P0.xu = np.full(n, -np.inf), np.full(n, np.inf)
    if "ball" not in cons:
        P0.R2 = None
    else:
        P0.R2 = 1.02 * float(x0 @ x0)                                # (the start is inside; the anchors lie outside)
    return G, n, m, delta, x0, anchor, a, P0


def _oracle_runs(key):
    """The oracle's run and its run from one ulp away; once per case, shared by the emulator and GPU runs, read-only."""
    if key not in _ORACLE_RUNS:
        name, pair_kind, spacing, cons = key
        G, n, m, delta, x0, anchor, a, P0 = _opt_case(*key)
        phi, d1, d2 = _sep_host(1, a, anchor)
        pair = _PairNp(G, np.ones(len(G.pi)), pair_kind, delta, KAPPA)
        ball = P0.R2 is not None
        curv, rmin = [], []

        def f(x):
            return float(np.sum(phi(x[:n]))) + pair.f(x)

        def grad_(g, x):
            g[:n] = d1(x[:n]) + pair.grad(x)

        def hlv_(dest, src, x, lam):
            dest[:] = (d2(x) + (2.0 * lam[m] if ball else 0.0)) * src + pair.hess_mul(x, src)
            if np.any(src):                                            # (projcg! starts from A 0)
                curv.append(float(src @ dest) / float(src @ src))
            rmin.append(float(np.sqrt(np.sum(pair._t(x) ** 2, axis=1)).min()) / delta)

        def oracle(xs, trace):
            p = R.LFPSQPParams(disp=R.DisplayOption.off, **_PAR)
            dv0 = P0.derivatives()
            if ball:
                return R.optimize(f, P0.c_, P0.d_, xs, P0.xl, P0.xu, m, 1, p,
                                  derivatives=R.Derivatives(grad_=grad_, hess_lag_vec_=hlv_, jac_c_=dv0.jac_c_, jac_d_=dv0.jac_d_), trace=trace)
            return R.optimize(f, P0.c_, xs, P0.xl, P0.xu, m, p, derivatives=R.Derivatives(grad_=grad_, hess_lag_vec_=hlv_, jac_c_=dv0.jac_c_), trace=trace)
        tr0, tr1 = [], []
        xr, objr, lamr, tir = oracle(x0, tr0)
        c0, r0 = min(curv), min(rmin)
        oracle(np.nextafter(x0, np.inf), tr1)
        sens = [np.linalg.norm(p['x'] - q['x']) / np.linalg.norm(q['x']) for p, q in zip(tr1, tr0)] + [np.inf] * (len(tr0) - len(tr1))
        _ORACLE_RUNS[key] = (tr0, xr, objr, tir, sens, c0, r0)
    return _ORACLE_RUNS[key]


@pytest.mark.parametrize("name,pair_kind,spacing,cons", _OPT_CASES)
def test_point_potential_objective_follows_the_oracle(dev_ctx, name, pair_kind, spacing, cons):
    """PointPotentialLinear through `optimize`: every truncated-Newton solve runs a SparseOperator on lfpsqp_projcg_sparse, on values refreshed at
    the current x, and the trajectory is the oracle's with numpy closures over the edge list for f, grad! and hess_lag_vec!.  Structure, spies and
    the one-ulp sensitivity rule are those of tests/test_sphess_edge.py::test_graph_potential_objective_follows_the_oracle.  Kind 2 (convex) in 2-D
    with ball and box and in 3-D with the box; kind 1 on a lattice stretched to 1.5 rest lengths with the ball, where, ON THE ORACLE ALONE, every
    product d'Ad of the run is positive (smallest Rayleigh quotient printed) and no edge gets shorter than its rest length: no solve leaves through
    the negative-curvature branch, which last bits would choose."""
    ctx = dev_ctx
    key = (name, pair_kind, spacing, cons)
    G, n, m, delta, x0, anchor, a, P0 = _opt_case(*key)
    tr0, xr, objr, tir, sens, cmin, rmin = _oracle_runs(key)
    print(f"[point potential {name} kind {pair_kind} {cons}] oracle alone: smallest d'Ad / d'd {cmin:.3e}, shortest edge {rmin:.3f} delta")
    assert cmin > 0.0
    if pair_kind == 1:
        assert rmin > 1.0
    ball = P0.R2 is not None
    p = 1 if ball else 0
    kw = dict(R2=P0.R2) if ball else {}
    if "box" in cons:
        kw.update(xl=P0.xl, xu=P0.xu)
    P = L.PointPotentialLinear(ctx, G.npoints, G.dim, m, ctx.matrix(n + p, m + p).hash_fill(1, 0, n, 1.0, n, m), P0.eq.b, 1, a, anchor,
                               edges=(G.pi, G.pj, 1.0), kappa=KAPPA, pair_kind=pair_kind, delta=delta, **kw)
    S = P.sparse_hessian
    assert (S.n, S.npoints, S.dim, S.row_width) == (n + p, G.npoints, G.dim, G.dim - 1 + G.dim * G.deg)       # (the slack row has no couplings)
    assert P.weights.h != S.h and (P.n, P.N) == (n, n + p)
    OPT = sys.modules["lfpsqp_jl_amd.optimize"]
    seen, rcs, orig = [], [], OPT.projcg_
    c_entry = ctx.L.lfpsqp_projcg_sparse
    tr = []

    def spy(*args, **kw_):
        seen.append((type(args[2]).__name__, bool(kw_.get("start_given")), args[2].S is S))
        return orig(*args, **kw_)

    def c_spy(*args):
        rc = c_entry(*args)
        rcs.append(rc)
        return rc
    OPT.projcg_ = spy
    setattr(ctx.L, "lfpsqp_projcg_sparse", c_spy)
    try:
        x, obj, lam, ti = P.optimize(x0, L.LFPSQPParams(disp=L.DisplayOption.off, **_PAR), trace=tr)
    finally:
        OPT.projcg_ = orig
        setattr(ctx.L, "lfpsqp_projcg_sparse", c_entry)
    assert seen and all(s == ("SparseOperator", True, True) for s in seen)
    assert len(rcs) == len(seen) and all(rc == 0 for rc in rcs)
    assert ti.iter == tir.iter and ti.condition.name == tir.condition.name
    print(f"[point potential {name} kind {pair_kind} {cons}] Newton-system iterations", [t.get('tn_iter') for t in tr0])
    assert any((t.get('tn_iter') or 0) >= 2 for t in tr0)
    rtol = max(1e-10, 10.0 * max(sens))
    _note(f"point potential {name} kind {pair_kind} {cons}: the oracle's one-ulp sensitivity {max(sens):.1e}")
    assert max(sens) <= 1e-12
    assert _compare_traces(tr, tr0, rtol=rtol) is None
    assert abs(obj[-1] - objr[-1]) <= 1e-11 * abs(objr[-1])
    assert np.linalg.norm(x - xr) <= 1e-10 * np.linalg.norm(xr)


# ---- 8. a size at which a workgroup of the vector launches takes several rounds ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", [((188, 189), 2), ((29, 29, 28), 1)])
def test_pair_eval_at_a_size_of_several_rounds(gpu_lib, shape, kind):
    """About 71 000 scalar rows, as tests/test_sphess_edge.py::test_edge_eval_at_a_size_of_several_rounds (138 or 139 tiles of the vector launches), one
    row behind the points: a refresh with f, grad and diag against numpy float64 with the kernel's expressions.  numpy rounds as often as the
    device does, so every bound of item 2 is taken TWICE, as there: rows within 2 gamma_{deg + count(a) + 3} sum |terms| (grad) and
    2 gamma_{deg + CV + 1} (diag); f against math.fsum of numpy's terms (no summation error on that side) within
    (gamma_{npoints deg + count(psi) + 1} + gamma_{count(psi)}) sum |terms|; H through one product with a hash vector v, rows within
    2 gamma_{Kr + deg + CV + 1} sum_j |H_ij| |v_j| with |H_ij| the magnitude sums of item 2 (an entry carries at most deg + CV + 1, the one inside
    a point; the fma chain Kr)."""
    ctx = L.Context(0, gpu_lib)
    try:
        npts, edges, base, delta = _lattice(shape)
        dim = len(shape)
        pi, pj = (np.ascontiguousarray(a) for a in np.array(edges, dtype=np.int64).T)
        nr, n, deg = dim * npts, dim * npts + 1, 2 * dim
        assert 70000 <= nr <= 72000
        w = 0.5 + synth.hash_vector(51, len(pi)) ** 2
        xh = np.concatenate([(base + 0.4 * (synth.hash_vector(52, nr).reshape(npts, dim) - 0.5)).ravel(), [7.0]])
        cpsi, ca, cv = _counts(kind, dim)
        W = L.SparseHessian.from_points(ctx, n, npts, dim, pi, pj, w)
        H = W.like()
        kr = W.row_width
        assert kr == dim - 1 + dim * deg
        x, g, d = ctx.vector(n, xh), ctx.vector(n), ctx.vector(n)
        f = W.pair_eval(kind, delta, KAPPA, x, g, d, H)
        assert W.pair_eval(kind, delta, KAPPA, x) == f               # (the same reduction from either kernel)
        X = xh[:nr].reshape(npts, dim)
        T = X[pi] - X[pj]
        psi, a, b = _pair_np(kind, T, delta)
        sw = KAPPA * w
        r = np.sqrt(np.sum(T * T, axis=1))
        amag, pmag = (1.0 + delta / r, 0.5 * (r + delta) ** 2) if kind == 1 else (a, psi)

        def scat(V, sign):
            out = np.zeros((npts, dim))
            np.add.at(out, pi, V)
            np.add.at(out, pj, sign * V)
            return out.ravel()
        eg = np.abs(g.download()[:nr] - scat((sw * a)[:, None] * T, -1.0)) / scat((sw * amag)[:, None] * np.abs(T), 1.0)
        ed = np.abs(d.download()[:nr] - scat(sw[:, None] * (a[:, None] + b[:, None] * T * T), 1.0)) / scat(sw[:, None] * (amag[:, None] + np.abs(b)[:, None] * T * T), 1.0)
        f_np, f_mag = math.fsum((sw * psi).tolist()), math.fsum((sw * pmag).tolist())
        vh = synth.hash_vector(7, n)
        V = vh[:nr].reshape(npts, dim)
        B = sw[:, None, None] * (a[:, None, None] * np.eye(dim)[None] + b[:, None, None] * (T[:, :, None] * T[:, None, :]))
        Bm = sw[:, None, None] * (amag[:, None, None] * np.eye(dim)[None] + np.abs(b)[:, None, None] * np.abs(T[:, :, None] * T[:, None, :]))
        off = lambda M: M * (1.0 - np.eye(dim))[None]
        ref = np.zeros((npts, dim))
        mag = np.zeros((npts, dim))
        for P_, Q_ in ((pi, pj), (pj, pi)):
            np.add.at(ref, P_, -np.einsum('eab,eb->ea', B, V[Q_]) + np.einsum('eab,eb->ea', off(B), V[P_]))
            np.add.at(mag, P_, np.einsum('eab,eb->ea', Bm, np.abs(V[Q_])) + np.einsum('eab,eb->ea', off(Bm), np.abs(V[P_])))
        got = _mul(ctx, H, vh)
        eh = np.abs(got[:nr] - ref.ravel()) / mag.ravel()
        bg, bd, bf, bh = 2 * _g(deg + ca + 3), 2 * _g(deg + cv + 1), _g(npts * deg + cpsi + 1) + _g(cpsi), 2 * _g(kr + deg + cv + 1)
        print(f"[pair eval {nr}] kind {kind} dim {dim}: grad {eg.max() / bg:.3f} of {bg:.2e}, diag {ed.max() / bd:.3f} of {bd:.2e}, "
              f"f {abs(f - f_np) / f_mag / bf:.4f} of {bf:.2e}, H v {eh.max() / bh:.3f} of {bh:.2e}")
        assert eg.max() <= bg and ed.max() <= bd
        assert abs(f - f_np) <= bf * f_mag
        assert eh.max() <= bh
        assert got[nr] == 0.0 and g.download()[nr] == 0.0 and d.download()[nr] == 0.0
    finally:
        ctx.close()
