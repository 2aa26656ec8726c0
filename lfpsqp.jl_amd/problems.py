"""Problem front-ends of ``optimize``.

* :class:`QuadLinearBallBox` -- the device-resident problem class of BASELINE configs 2-5:
  f = ||x - xc||^2, dense linear equalities J x = b, optional ball x'x <= R2 (turned into an
  equality with a slack variable exactly as src/optimize.jl:23-51 does) and optional box bounds.
  f, grad!, c!, jac! and the (diagonal) Lagrangian Hessian all run on the device.
* :func:`optimize` -- the reference's method table (src/optimize.jl:13,83,88,107,112,119) for
  arbitrary HOST callables: the "host-callback fallback".  Iterates are downloaded for every user
  call, so it is for plumbing / small problems (config 1), not for the 1e7-variable configs.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from .device import Context, DeviceMatrix, DeviceVector
from .optimize import optimize_core
from .params import LFPSQPParams
from .retractions import DeviceConstraints


class QuadLinearBallBox:
    def __init__(self, ctx: Context, n: int, m: int, Jct: DeviceMatrix, b, R2: Optional[float] = None, xl=None, xu=None,
                 xc: float = 0.0, n_global: Optional[int] = None, owns_slack: bool = True, Jsp=None):
        """n = rows of this rank's shard.  Jct: device matrix with n + ploc rows and m + p columns
        (p = 1 iff R2 is given; ploc = 1 on the rank that owns the slack variable -- the last one --
        else 0) whose leading n x m block holds the constraint gradients; the slack row and the ball
        column are managed here."""
        self.ctx, self.n, self.m, self.xc = ctx, n, m, float(xc)
        self.p = 0 if R2 is None else 1
        self.ploc = self.p if owns_slack else 0
        self.N, self.M = n + self.ploc, m + self.p
        assert Jct.n == self.N and Jct.m == self.M
        self.Jct = Jct
        self.R2 = 0.0 if R2 is None else float(R2)
        # Jsp: optional SparseMatrix (N x m) with the entries of the linear block Jct[:, :m]: c! and ProjPenalty's inner solves
        # then stream its nonzeros (the tangent setup and the Newton retraction keep the dense block)
        self.cons = DeviceConstraints(Jct, m, b, has_ball=self.p == 1, R2=self.R2, n_x=n, slack_row=n if self.ploc else -1, Jsp=Jsp)
        self.xl = None if xl is None else np.asarray(xl, dtype=np.float64)
        self.xu = None if xu is None else np.asarray(xu, dtype=np.float64)
        self.n_global = n if n_global is None else n_global
        self.is_diagonal = True
        # grad^2 of the Lagrangian is 2 I when there is no ball: the truncated-Newton solve converges in ONE projected-CG iteration (config 3).
        # optimize then takes its first allocations instead of placing the work vectors by trial (tens of ms that a handful of iterations
        # cannot repay)
        self.scalar_hessian = self.p == 0 and type(self) is QuadLinearBallBox

    # -- callbacks in the contract of optimize_core -------------------------------------------
    def f(self, x: DeviceVector) -> float:
        out = C.c_double()
        self.ctx.check(self.ctx.L.lfpsqp_sumsq_shift(self.ctx.h, x.h, self.n, self.xc, C.byref(out)))
        return out.value

    def grad_(self, g: DeviceVector, x: DeviceVector):
        self.ctx.check(self.ctx.L.lfpsqp_affine_head(self.ctx.h, 2.0, x.h, -2.0 * self.xc, self.n, g.h))

    def jac_(self, Jct, cval, x):
        return self.cons.jac_(Jct, cval, x)

    def diag_objective_(self, hx: DeviceVector, x: DeviceVector):
        """The objective's part of the diagonal Lagrangian Hessian; the constraints' part is ``self.cons.hess_diag_`` -- the split
        ``optimize`` uses to fold the latter into its tangent-step pass (lfpsqp_tangent_step): diag_ == diag_objective_ + cons.hess_diag_."""
        L = self.ctx.L
        self.ctx.check(L.lfpsqp_vec_fill_range(self.ctx.h, hx.h, 0, self.n, 2.0))
        if self.ploc:
            self.ctx.check(L.lfpsqp_vec_fill_range(self.ctx.h, hx.h, self.n, 1, 0.0))

    def diag_(self, hx: DeviceVector, x: DeviceVector, lam: np.ndarray):
        """diag of grad^2 f + sum lam_i grad^2 c_i: 2 (+ 2 lam_ball) on the user's variables, 0 on the slack."""
        h = 2.0 + (2.0 * float(lam[self.m]) if self.p else 0.0)
        L = self.ctx.L
        self.ctx.check(L.lfpsqp_vec_fill_range(self.ctx.h, hx.h, 0, self.n, h))
        if self.ploc:
            self.ctx.check(L.lfpsqp_vec_fill_range(self.ctx.h, hx.h, self.n, 1, 0.0))

    # -- the slack transformation of src/optimize.jl:23-36 --------------------------------------
    def aux_start(self, x0):
        x0 = np.asarray(x0, dtype=np.float64)
        if not self.p:
            return x0, self.xl, self.xu
        tmp = self.ctx.vector(self.n, x0)                       # global x0'x0 (all-reduced over the shards)
        saved, self.xc = self.xc, 0.0
        xx = self.f(tmp) if self.n else self.f(self.ctx.vector(0))
        self.xc = saved
        tmp.free()
        xl = -np.inf * np.ones(self.n) if self.xl is None else self.xl
        xu = np.inf * np.ones(self.n) if self.xu is None else self.xu
        if not self.ploc:                                       # another rank owns the slack variable
            return x0, xl, xu
        return np.concatenate([x0, [xx - self.R2]]), np.concatenate([xl, [-np.inf]]), np.concatenate([xu, [0.0]])

    def optimize(self, x0, param: LFPSQPParams | None = None, trace=None):
        x0a, xl, xu = self.aux_start(x0)
        x, obj, lam, ti = optimize_core(self.f, self.grad_, self.cons, self.jac_, self, x0a, xl, xu, self.M, param, ctx=self.ctx,
                                        n_global=self.n_global + self.p, trace=trace)
        return x[:self.n], obj, lam, ti


class SeparableLinearBallBox(QuadLinearBallBox):
    """A second device-resident problem class: a SEPARABLE objective f(x) = sum_i phi(x_i - c_i; a_i) with per-variable
    parameters -- ``kind`` 0: a t^2, 1: a t^4 + t^2, 2: a (sqrt(1 + t^2) - 1) (pseudo-Huber) -- under the same constraint set as
    :class:`QuadLinearBallBox` (dense or sparse linear equalities, optional ball with slack, optional box).  f, grad! and the
    diagonal of the Lagrangian Hessian phi''(x_i) + 2 lam_ball are elementwise kernels (lfpsqp_separable), so the whole
    `optimize` run stays on the device and uses the fused projected-CG path; unlike the quadratic class the Hessian changes with x
    and the truncated-Newton solves take several iterations."""

    def __init__(self, ctx: Context, n: int, m: int, Jct: DeviceMatrix, b, kind: int, a, c=0.0, **kw):
        super().__init__(ctx, n, m, Jct, b, **kw)
        self.kind = int(kind)
        self.a_dev = None if np.isscalar(a) else ctx.vector(n, np.asarray(a, dtype=np.float64))
        self.c_dev = None if np.isscalar(c) else ctx.vector(n, np.asarray(c, dtype=np.float64))
        self.a0 = float(a) if np.isscalar(a) else 0.0
        self.c0 = float(c) if np.isscalar(c) else 0.0

    def _sep(self, mode, x, out_vec=None):
        out = C.c_double()
        L = self.ctx.L
        self.ctx.check(L.lfpsqp_separable(self.ctx.h, self.kind, mode, self.a_dev.h if self.a_dev is not None else None, self.a0,
                                          self.c_dev.h if self.c_dev is not None else None, self.c0, x.h, self.n,
                                          out_vec.h if out_vec is not None else None, C.byref(out)))
        return out.value

    def f(self, x: DeviceVector) -> float:
        return self._sep(0, x)

    def grad_(self, g: DeviceVector, x: DeviceVector):
        self._sep(1, x, g)
        if self.ploc:
            self.ctx.check(self.ctx.L.lfpsqp_vec_fill_range(self.ctx.h, g.h, self.n, 1, 0.0))      # the slack variable is not in f

    def diag_objective_(self, hx: DeviceVector, x: DeviceVector):
        self._sep(2, x, hx)
        if self.ploc:
            self.ctx.check(self.ctx.L.lfpsqp_vec_fill_range(self.ctx.h, hx.h, self.n, 1, 0.0))

    def diag_(self, hx: DeviceVector, x: DeviceVector, lam: np.ndarray):
        self._sep(2, x, hx)
        if self.p:                                                                                  # + 2 lam_ball on the user's variables
            ones = getattr(self, "_lamvec", None)
            if ones is None:
                ones = self._lamvec = self.ctx.vector(hx.n)
            L = self.ctx.L
            self.ctx.check(L.lfpsqp_vec_fill_range(self.ctx.h, ones.h, 0, self.n, 2.0 * float(lam[self.m])))
            from .device import axpby
            axpby(1.0, ones, 1.0, hx)
        if self.ploc:
            self.ctx.check(self.ctx.L.lfpsqp_vec_fill_range(self.ctx.h, hx.h, self.n, 1, 0.0))

    def aux_start(self, x0):
        x0 = np.asarray(x0, dtype=np.float64)
        if not self.p:
            return x0, self.xl, self.xu
        tmp = self.ctx.vector(self.n, x0)                       # global x0'x0 through the quadratic kernel
        out = C.c_double()
        self.ctx.check(self.ctx.L.lfpsqp_sumsq_shift(self.ctx.h, tmp.h, self.n, 0.0, C.byref(out)))
        tmp.free()
        xl = -np.inf * np.ones(self.n) if self.xl is None else self.xl
        xu = np.inf * np.ones(self.n) if self.xu is None else self.xu
        if not self.ploc:
            return x0, xl, xu
        return np.concatenate([x0, [out.value - self.R2]]), np.concatenate([xl, [-np.inf]]), np.concatenate([xu, [0.0]])


def difference_band(n: int, order: int, kappa: float = 1.0):
    """The diagonal (length n) and the ``order`` off-diagonals (n x order, column k-1: entry i couples i and i+k; the last k entries zero) of
    kappa D'D, D the (n - order) x n matrix of ``order``-th forward differences (boundary rows included)."""
    from math import comb
    cf = np.array([(-1.0) ** (order - t) * comb(order, t) for t in range(order + 1)])       # row j of D: cf[t] at column j + t
    rows = max(n - order, 0)
    diag = np.zeros(n)
    off = np.zeros((n, order))
    for t in range(order + 1):
        diag[t:t + rows] += cf[t] * cf[t]
        for k in range(1, order + 1 - t):
            off[t:t + rows, k - 1] += cf[t] * cf[t + k]
    return kappa * diag, kappa * off


class _LaplacianSeparableLinear(SeparableLinearBallBox):
    """What :class:`ChainSeparableLinear`, :class:`GridSeparableLinear` and :class:`GraphSeparableLinear` share: a separable objective plus a
    quadratic term 1/2 x'(kappa L)x with a CONSTANT symmetric kappa L.  A subclass sets ``_deg`` (device, N entries: the diagonal of kappa L, zero
    on the slack row) and its couplings, defines ``_operator(dg)`` -- kappa L as a coupled operator with the diagonal ``dg`` -- and ends its
    constructor with ``_init_laplacian()``."""

    def _init_laplacian(self):
        self._lap = self._operator(self._deg)
        self._tmp = self.ctx.vector(self.N)
        self._lap2 = self._tmp2 = None                                    # the same over stacked iterates [x | gap | y] (bounds): zero on the y half

    def _smooth(self, x: DeviceVector):
        """tmp = kappa L x (x plain, or stacked: the x half)."""
        if x.n == self.N:
            return self._lap.mul_(self._tmp, x)
        if self._lap2 is None:
            from .inequality import StackedVector
            deg2 = StackedVector(self.ctx, self.N)
            deg2.copy_range_from(self._deg, self.N)
            self._lap2 = self._operator(deg2)
            self._tmp2 = StackedVector(self.ctx, self.N)
        return self._lap2.mul_(self._tmp2, x)

    def f(self, x: DeviceVector) -> float:
        from .device import dot
        return super().f(x) + 0.5 * dot(x, self._smooth(x))

    def grad_(self, g: DeviceVector, x: DeviceVector):
        from .device import axpby
        super().grad_(g, x)
        axpby(1.0, self._smooth(x), 1.0, g)

    def diag_objective_(self, hx: DeviceVector, x: DeviceVector):
        from .device import axpby
        super().diag_objective_(hx, x)
        axpby(1.0, self._deg, 1.0, hx)

    def diag_(self, hx: DeviceVector, x: DeviceVector, lam: np.ndarray):
        from .device import axpby
        super().diag_(hx, x, lam)
        axpby(1.0, self._deg, 1.0, hx)


class ChainSeparableLinear(_LaplacianSeparableLinear):
    """A separable objective plus a CHAIN term: f(x) = sum_i phi(x_i - c_i; a_i) + kappa/2 ||D^r x||^2, D^r the r-th forward difference over the n
    user variables (``order`` r = 1 .. 4; r = 1: kappa/2 sum_{i<n-1} (x_{i+1} - x_i)^2, smoothing / first differences; r = 2: Whittaker /
    Hodrick-Prescott smoothing, curvature penalties -- the kind of objective whose Hessian the reference reaches only through hess_lag_vec!,
    src/autodiff_generators.jl:72-107) under dense linear equalities, with the optional ball (slack variable) and box bounds of
    :class:`QuadLinearBallBox`.  order = 1: the Lagrangian Hessian is TRIDIAGONAL: diagonal phi''(x_i) + kappa deg_i (+ 2 lam_ball; deg = 1 at
    the two ends, 2 inside), couplings -kappa; ``optimize`` hands it to projcg_ as a :class:`TridiagonalOperator` (``offdiag`` below; with
    bounds the augmented stacked diagonal next to the same couplings) and the truncated-Newton solves keep one pass over the basis per iteration
    (lfpsqp_projcg_tridiag).  order >= 2: the Hessian is BANDED with bandwidth r (the diagonal and the r off-diagonals of kappa D^r'D^r,
    :func:`difference_band`, built once on the host): ``offdiags`` (N x r device matrix) and a :class:`BandedOperator` on lfpsqp_projcg_band.
    The slack row, when the ball is there, has no chain term.  One rank (the couplings would cross the shard boundaries)."""

    def __init__(self, ctx: Context, n: int, m: int, Jct: DeviceMatrix, b, kind: int, a, c=0.0, kappa: float = 1.0, order: int = 1, **kw):
        assert kw.get("n_global", n) in (None, n), "chain objective: one rank (the couplings would cross the shard boundaries)"
        assert int(order) in (1, 2, 3, 4), "chain objective: order 1 .. 4"
        super().__init__(ctx, n, m, Jct, b, kind, a, c, **kw)
        self.kappa = float(kappa)
        self.order = int(order)
        N = self.N                                                        # n, or n + 1 with the ball's slack variable (no chain term on it)
        deg = np.zeros(N)
        if self.order == 1:
            deg[:n] = 2.0 * self.kappa
            deg[0] = deg[n - 1] = self.kappa if n > 1 else 0.0
            off = np.full(N, -self.kappa)
            off[n - 1:] = 0.0                                             # (entry n-1 would couple the last variable to the slack row; N-1 is ignored)
            self._deg = ctx.vector(N, deg)
            self.offdiag = ctx.vector(N, off)
        else:
            offs = np.zeros((N, self.order), order='F')
            deg[:n], offs[:n] = difference_band(n, self.order, self.kappa)   # (entries i + k >= n are zero: no coupling to the slack row)
            self._deg = ctx.vector(N, deg)
            self.offdiags = ctx.matrix(N, self.order, offs)
        self._init_laplacian()

    def _operator(self, dg):
        from .projcg import BandedOperator, TridiagonalOperator
        if self.order == 1:
            return TridiagonalOperator(0.0, dg, self.offdiag)            # kappa * L, L = the path graph's Laplacian
        return BandedOperator(0.0, dg, self.offdiags, self.order)        # kappa D'D


def graph_diagonals(n: int, i, j, w):
    """The weighted graph Laplacian of an edge list as the arrays of a :class:`DiagonalsOperator`: for edges (i_e, j_e), i_e < j_e < n, with weights
    w_e (a scalar or one per edge) -- the Hessian of 1/2 sum_e w_e (x_i - x_j)^2 -- returns ``(diag, off, dists)``: ``diag[i] += w``, ``diag[j] += w``
    and ``off[i, column of distance j - i] -= w`` per edge, ``dists`` the distinct distances j - i in increasing order, ``off`` n x K in Fortran
    order with zeros wherever no edge put a value (the ignored tails i + s_k >= n among them).  Repeated edges add up.  More than 13 distinct
    distances do not fit one operator: ValueError."""
    n = int(n)
    i, j = np.asarray(i, dtype=np.int64).ravel(), np.asarray(j, dtype=np.int64).ravel()
    w = np.broadcast_to(np.asarray(w, dtype=float), i.shape)
    assert i.shape == j.shape and i.size >= 1, "graph_diagonals: at least one edge"
    assert np.all((0 <= i) & (i < j) & (j < n)), "graph_diagonals: edges (i, j) with 0 <= i < j < n"
    d = j - i
    dists = np.flatnonzero(np.bincount(d, minlength=2))                # (counting, not sorting: the edge list of a 1e7-point volume has 1.3e8 entries)
    if len(dists) > 13:
        raise ValueError(f"graph_diagonals: {len(dists)} distinct distances j - i, at most 13 off-diagonals fit one operator")
    diag = np.bincount(i, w, n) + np.bincount(j, w, n)
    off = 0.0 - np.bincount(i + np.searchsorted(dists, d) * n, w, n * len(dists)).reshape((n, len(dists)), order='F')
    return diag, off, tuple(int(s) for s in dists)


def grid_edges(shape, periodic=False, corners: bool = False):
    """(i, j), i < j: the edges of the grid graph of a field of ``shape`` in row-major numbering, as two index arrays -- the edge list behind
    :func:`grid_laplacian`, for :func:`graph_diagonals`, :class:`SparseHessian` and :class:`GraphSeparableLinear`.  ``periodic`` (a bool, or one
    per axis) closes an axis on itself (it needs at least 3 points); ``corners`` joins every pair of points whose indices differ by at most 1
    along every axis.  Any number of axes; no limit on the distances j - i that arise."""
    shape = tuple(int(s) for s in shape)
    per = (bool(periodic),) * len(shape) if np.ndim(periodic) == 0 else tuple(bool(p) for p in periodic)
    assert len(per) == len(shape), "grid_edges: periodic is a bool or one bool per axis"
    assert all(s >= 1 for s in shape) and int(np.prod(shape)) > 1, "grid_edges: a grid of more than one point"
    assert all(s >= 3 for s, p in zip(shape, per) if p), "grid_edges: a periodic axis needs at least 3 points"
    return _grid_edges(shape, per, bool(corners))


def _grid_edges(shape, periodic, corners):
    """(i, j), i < j: the edges of the grid graph in row-major numbering.  Every offset in {-1, 0, 1}^d (corners) or along one axis whose first
    nonzero component is +1 names each edge once; a periodic axis wraps, any other drops the neighbours beyond its end."""
    import itertools
    d = len(shape)
    if corners:
        offsets = [o for o in itertools.product((-1, 0, 1), repeat=d) if next((c for c in o if c), 0) > 0]
    else:
        offsets = [tuple(int(ax == k) for k in range(d)) for ax in range(d)]
    coords = np.indices(shape).reshape(d, -1)
    flat = np.arange(coords.shape[1])
    ii, jj = [], []
    for o in offsets:
        keep = np.ones(len(flat), dtype=bool)
        nb = []
        for ax in range(d):
            c = coords[ax] + o[ax]
            if periodic[ax]:
                c = c % shape[ax]
            else:
                keep &= (c >= 0) & (c < shape[ax])
            nb.append(c)
        if not keep.any():
            continue
        q = np.ravel_multi_index([c[keep] for c in nb], shape)
        ii.append(np.minimum(flat[keep], q))
        jj.append(np.maximum(flat[keep], q))
    return np.concatenate(ii), np.concatenate(jj)


def grid_laplacian(shape, kappa: float = 1.0, periodic=False, corners: bool = False):
    """kappa L for the grid graph of a 2-D or 3-D field stored in row-major order (last axis fastest), L = D - W its Laplacian (edges between
    neighbours along each axis): returns ``(diag, off, dists)`` -- the diagonal kappa deg_i (length n = prod(shape)), the couplings (n x K,
    column k: entry i couples points i and i + dists[k]; -kappa on an edge, 0 where i is the last point along that axis) and the distances
    (1, n_last, n_last n_mid ...) in increasing order; axes of length 1 have no edges and no column.
    ``periodic`` (a bool, or one per axis): the axis closes on itself -- its wrap-around edge between rows i < j is one more entry at distance
    j - i (2-D: distances (1, nx - 1, nx, (ny - 1) nx)); the axis needs at least 3 points (with 2 the wrap would repeat the one edge).
    ``corners``: every pair of points whose indices differ by at most 1 along every axis is an edge of weight kappa -- 8 neighbours in 2-D
    (4 distances), 26 in 3-D (13).  Both variants are built through :func:`graph_diagonals`, which raises ValueError where more than 13 distances
    arise (a periodic 3-D grid with corners)."""
    shape = tuple(int(s) for s in shape)
    assert len(shape) in (2, 3) and all(s >= 1 for s in shape)
    n = int(np.prod(shape))
    per = (bool(periodic),) * len(shape) if np.ndim(periodic) == 0 else tuple(bool(p) for p in periodic)
    assert len(per) == len(shape), "grid_laplacian: periodic is a bool or one bool per axis"
    if any(per) or corners:
        assert all(s >= 3 for s, p in zip(shape, per) if p), "grid_laplacian: a periodic axis needs at least 3 points"
        assert n > 1, "grid_laplacian: a grid of more than one point"
        return graph_diagonals(n, *_grid_edges(shape, per, bool(corners)), float(kappa))
    idx = np.arange(n).reshape(shape)
    diag = np.zeros(n)
    cols, dists = [], []
    stride = 1
    for ax in range(len(shape) - 1, -1, -1):                    # last axis first: increasing distances
        if shape[ax] > 1:
            lo = np.take(idx, np.arange(shape[ax] - 1), axis=ax).ravel()     # the points with a neighbour further along this axis
            col = np.zeros(n)
            col[lo] = -kappa
            diag[lo] += kappa
            diag[lo + stride] += kappa
            cols.append(col)
            dists.append(stride)
        stride *= shape[ax]
    assert cols, "grid_laplacian: a grid of more than one point"
    return diag, np.asfortranarray(np.stack(cols, axis=1)), tuple(dists)


class GridSeparableLinear(_LaplacianSeparableLinear):
    """A separable objective plus a GRID smoothness term: f(x) = sum_i phi(x_i - c_i; a_i) + kappa/2 sum_{grid edges (i,j)} (x_i - x_j)^2 over a
    2-D or 3-D field of ``shape`` in row-major order (an image, a volume: diffusion / Tikhonov smoothing) under dense linear equalities, with the
    optional ball (slack variable) and box bounds of :class:`QuadLinearBallBox`.  The Lagrangian Hessian is a diagonal, phi''(x_i) + kappa deg_i
    (+ 2 lam_ball), plus one off-diagonal per axis FAR from the main one (distances 1, nx, nx ny: :func:`grid_laplacian`): ``diagonals`` =
    (dists, off) below, and ``optimize`` hands it to projcg_ as a :class:`DiagonalsOperator` -- the truncated-Newton solves keep one pass over
    the basis per iteration (lfpsqp_projcg_diags; with bounds the augmented stacked diagonal next to the same couplings).  ``periodic`` and
    ``corners`` are those of :func:`grid_laplacian`: a torus, and the 9- / 27-point neighbourhood (up to 13 off-diagonals:
    lfpsqp_projcg_stencil).  The slack row, when the ball is there, has no couplings.  One rank (the couplings would cross the shard
    boundaries)."""

    def __init__(self, ctx: Context, shape, m: int, Jct: DeviceMatrix, b, kind: int, a, c=0.0, kappa: float = 1.0, periodic=False,
                 corners: bool = False, **kw):
        n = int(np.prod(shape))
        assert kw.get("n_global", n) in (None, n), "grid objective: one rank (the couplings would cross the shard boundaries)"
        super().__init__(ctx, n, m, Jct, b, kind, a, c, **kw)
        self.shape = tuple(int(s) for s in shape)
        self.kappa = float(kappa)
        N = self.N                                                        # n, or n + 1 with the ball's slack variable (no coupling to it)
        deg_h, off_h, dists = grid_laplacian(self.shape, self.kappa, periodic, corners)
        deg = np.zeros(N)
        off = np.zeros((N, len(dists)), order='F')
        deg[:n], off[:n] = deg_h, off_h
        self._deg = ctx.vector(N, deg)
        self.diagonals = (dists, ctx.matrix(N, len(dists), off))
        self._init_laplacian()

    def _operator(self, dg):
        from .projcg import DiagonalsOperator
        return DiagonalsOperator(0.0, dg, self.diagonals[1], self.diagonals[0])      # kappa L


class GraphSeparableLinear(_LaplacianSeparableLinear):
    """A separable objective plus a smoothness term on an arbitrary GRAPH: f(x) = sum_i phi(x_i - c_i; a_i) + kappa/2 sum_e w_e (x_i - x_j)^2 over
    the undirected edges ``edges = (i, j, w)`` (0-based index arrays, ``w`` a scalar or one weight per edge; repeated edges add up) -- a triangle
    mesh, a k-nearest-neighbour graph, a grid in any numbering, at most 32 neighbours per vertex -- under dense linear equalities, with the optional
    ball (slack variable) and box bounds of :class:`QuadLinearBallBox`.  The Lagrangian Hessian is a diagonal, phi''(x_i) + kappa (weighted degree)_i
    (+ 2 lam_ball), plus the entries -kappa w_e: ``sparse_hessian`` below (a :class:`SparseHessian` of N rows; the slack row, when the ball is
    there, has no couplings), and ``optimize`` hands it to projcg_ as a :class:`SparseOperator` -- the truncated-Newton solves keep one pass over the
    basis per iteration (lfpsqp_projcg_sparse; with bounds the augmented stacked diagonal next to the same couplings).  One rank (the couplings
    would cross the shard boundaries)."""

    def __init__(self, ctx: Context, n: int, m: int, Jct: DeviceMatrix, b, kind: int, a, c=0.0, edges=None, kappa: float = 1.0, **kw):
        assert kw.get("n_global", n) in (None, n), "graph objective: one rank (the couplings would cross the shard boundaries)"
        assert edges is not None and len(edges) == 3, "graph objective: edges = (i, j, w)"
        super().__init__(ctx, n, m, Jct, b, kind, a, c, **kw)
        from .projcg import SparseHessian
        self.kappa = float(kappa)
        N = self.N                                                        # n, or n + 1 with the ball's slack variable (no coupling to it)
        ei, ej, w = _edge_list(edges, n, "graph objective: edges between the n variables")
        w = self.kappa * w
        deg = np.zeros(N)
        deg[:n] = np.bincount(ei, w, n) + np.bincount(ej, w, n)
        self._deg = ctx.vector(N, deg)
        self.sparse_hessian = SparseHessian(ctx, N, ei, ej, -w)
        self._init_laplacian()

    def _operator(self, dg):
        from .projcg import SparseOperator
        return SparseOperator(0.0, dg, self.sparse_hessian)               # kappa L


def _edge_list(edges, count: int, what: str):
    """``edges = (i, j, w)`` as two int64 index arrays below ``count`` and one weight per edge (``w`` a scalar or an array)."""
    ei, ej = (np.asarray(e, dtype=np.int64).ravel() for e in edges[:2])
    assert ei.shape == ej.shape and np.all((0 <= ei) & (ei < count) & (0 <= ej) & (ej < count)), what
    return ei, ej, np.broadcast_to(np.asarray(edges[2], dtype=np.float64), ei.shape)


class _PotentialSeparableLinear(SeparableLinearBallBox):
    """What :class:`GraphPotentialLinear` and :class:`PointPotentialLinear` share: a separable objective plus a term whose Hessian lives on a fixed
    sparse pattern and changes with x.  A subclass builds ``weights`` (a :class:`SparseHessian`, never modified) and defines ``_term``: the
    evaluator of ``weights`` with the term's parameters bound; ``sparse_hessian`` = ``weights.like()`` holds the current entries."""

    def _init_potential(self, weights):
        self.weights = weights
        self.sparse_hessian = weights.like()

    def f(self, x: DeviceVector) -> float:
        return super().f(x) + self._term(x, want_f=True)

    def grad_(self, g: DeviceVector, x: DeviceVector):
        super().grad_(g, x)
        self._term(x, grad=g)

    def diag_objective_(self, hx: DeviceVector, x: DeviceVector):
        super().diag_objective_(hx, x)
        self._term(x, diag=hx, out=self.sparse_hessian)

    def diag_(self, hx: DeviceVector, x: DeviceVector, lam: np.ndarray):
        super().diag_(hx, x, lam)
        self._term(x, diag=hx, out=self.sparse_hessian)


class GraphPotentialLinear(_PotentialSeparableLinear):
    """A separable objective plus a NON-QUADRATIC edge term on a graph: f(x) = sum_i phi(x_i - c_i; a_i) + kappa sum_e w_e psi(x_i - x_j; delta) over
    the undirected edges ``edges = (i, j, w)`` of :class:`GraphSeparableLinear` -- ``edge_kind`` 0: psi = t^2/2 (that class's term), 1: t^2/2 +
    t^4/4 (stiffening), 2: the pseudo-Huber function delta^2 (sqrt(1 + (t/delta)^2) - 1) (edge-preserving smoothing) -- under the same constraint
    set (dense linear equalities, optional ball with its slack row, optional box).  The Lagrangian Hessian has the graph's pattern and values that
    CHANGE with x: the diagonal phi''(x_i) + kappa sum_j w_ij psi''(x_i - x_j) (+ 2 lam_ball) and the entries -kappa w_e psi''(x_i - x_j).
    ``weights`` holds w (a :class:`SparseHessian` of N rows, never modified) and ``sparse_hessian`` = ``weights.like()`` the current entries:
    ``diag_objective_`` / ``diag_`` -- ``optimize`` calls one of them at the current x before every truncated-Newton solve -- add the diagonal
    and rewrite ``sparse_hessian`` in the same device call (lfpsqp_sphess_edge_eval), so ``optimize`` runs it as a :class:`SparseOperator` on
    lfpsqp_projcg_sparse exactly as it runs the constant class; f is the kernel that only reads.  One rank.  For a graph whose numbering has no
    locality set ``ctx.options.tridiagonal_one_pass = False`` (``SparseOperator.fused = False``), as FINDINGS.md 19 advises for the constant
    class: the gathers of the solve, and of this evaluation, then fetch a cache line per value either way."""

    def __init__(self, ctx: Context, n: int, m: int, Jct: DeviceMatrix, b, kind: int, a, c=0.0, edges=None, kappa: float = 1.0, edge_kind: int = 2,
                 delta: float = 1.0, **kw):
        assert kw.get("n_global", n) in (None, n), "graph objective: one rank (the couplings would cross the shard boundaries)"
        assert edges is not None and len(edges) == 3, "graph objective: edges = (i, j, w)"
        assert int(edge_kind) in (0, 1, 2), "graph objective: edge_kind 0 .. 2"
        super().__init__(ctx, n, m, Jct, b, kind, a, c, **kw)
        from .projcg import SparseHessian
        self.kappa, self.edge_kind, self.delta = float(kappa), int(edge_kind), float(delta)
        # N rows: the slack row, when the ball is there, has no edges
        self._init_potential(SparseHessian(ctx, self.N, *_edge_list(edges, n, "graph objective: edges between the n variables")))

    def _term(self, x, grad=None, diag=None, out=None, want_f=False):
        return self.weights.edge_eval(self.edge_kind, self.delta, self.kappa, x, grad, diag, out, want_f)


class PointPotentialLinear(_PotentialSeparableLinear):
    """A separable objective plus a PAIR potential between points of ``dim`` = 2 or 3 unknowns each: the n = dim*npoints variables are interleaved
    (x[dim*p + c] is component c of point p) and f(x) = sum_i phi(x_i - c_i; a_i) + kappa sum_e w_e psi(x_p - x_q; delta) over the undirected
    edges ``edges = (pi, pj, w)`` between POINTS -- ``pair_kind`` 0: psi = |t|^2/2, 1: (|t| - delta)^2/2 (a spring of rest length ``delta``: truss
    and spring networks, graph layout, sensor localisation), 2: the radial pseudo-Huber function delta^2 (sqrt(1 + |t|^2/delta^2) - 1)
    (vector-valued edge-preserving smoothing) -- under the constraint set of :class:`GraphPotentialLinear` (dense linear equalities, optional ball
    with its slack row, optional box), of which this class has the shape line for line.  Every edge contributes a dense dim x dim block
    a I + b t t' to the Lagrangian Hessian, every point the entries between its own components, and all of them change with x: ``weights``
    (:meth:`SparseHessian.from_points`, N rows, never modified) holds w, ``sparse_hessian`` = ``weights.like()`` the current entries, rewritten
    with the diagonal by ``diag_objective_`` / ``diag_`` in one device call (lfpsqp_sphess_pair_eval) before every truncated-Newton solve, which
    ``optimize`` then runs as a :class:`SparseOperator` on lfpsqp_projcg_sparse.  At most 15 neighbours per point in 2-D, 10 in 3-D.  Kind 1 is
    not convex where an edge is shorter than its rest length, and singular where two joined points coincide.  One rank.
    ``rest``: one value per edge, aligned with ``edges`` (every edge once) -- the rest length l_e of kind 1 (a truss bar's natural length, a
    measured distance), the delta_e of kind 2 -- which overrides ``delta`` on the edges.  ``anchors = (point, pos, u)`` or ``(point, pos, u,
    par)``: the fixed points of :class:`PointAnchors` (supports, beacons), the term kappa sum_k u_k psi(x_p - a_k; par_k) with ``delta`` where no
    ``par`` is given; at most 8 on a point.  Both are evaluated in the same device call (lfpsqp_sphess_pair_eval_ex)."""

    def __init__(self, ctx: Context, npoints: int, dim: int, m: int, Jct: DeviceMatrix, b, kind: int, a, c=0.0, edges=None, kappa: float = 1.0,
                 pair_kind: int = 2, delta: float = 1.0, rest=None, anchors=None, **kw):
        n = int(dim) * int(npoints)
        assert kw.get("n_global", n) in (None, n), "graph objective: one rank (the couplings would cross the shard boundaries)"
        assert edges is not None and len(edges) == 3, "point objective: edges = (pi, pj, w)"
        assert int(dim) in (2, 3), "point objective: dim 2 or 3"
        assert int(pair_kind) in (0, 1, 2), "point objective: pair_kind 0 .. 2"
        super().__init__(ctx, n, m, Jct, b, kind, a, c, **kw)
        from .projcg import PointAnchors, SparseHessian
        self.npoints, self.dim = int(npoints), int(dim)
        self.kappa, self.pair_kind, self.delta = float(kappa), int(pair_kind), float(delta)
        # N rows: the slack row, when the ball is there, has no edges
        ei, ej, w = _edge_list(edges, npoints, "point objective: edges between the points")
        self._init_potential(SparseHessian.from_points(ctx, self.N, self.npoints, self.dim, ei, ej, w))
        # one l (kind 1) or delta (kind 2) per edge, aligned with `edges`: overrides `delta` on the edges (every edge once: a parameter does not add up)
        self.params = None if rest is None else self.weights.point_values(ei, ej, rest)
        # anchors = (point, pos, u) or (point, pos, u, par): kappa sum_k u_k psi(x_p - a_k; par_k), without par with `delta`
        assert anchors is None or len(anchors) in (3, 4), "point objective: anchors = (point, pos, u) or (point, pos, u, par)"
        self.anchors = None if anchors is None else PointAnchors(self.weights, *anchors)

    def _term(self, x, grad=None, diag=None, out=None, want_f=False):
        return self.weights.pair_eval(self.pair_kind, self.delta, self.kappa, x, grad, diag, out, want_f, params=self.params, anchors=self.anchors)


class SeparableElementwiseBox(SeparableLinearBallBox):
    """The device-resident problem class with NONLINEAR equality constraints: a separable objective
    (``kind`` / ``a`` / ``c`` as in :class:`SeparableLinearBallBox`) under ``cons``, an :class:`ElementwiseConstraints`
    (c(x) = A' phi(x) + qw x'x - b: the reference's sin and sphere test systems and their relatives), with optional box
    bounds.  f, grad!, c!, jac! and the diagonal Lagrangian Hessian phi_f''(x) + phi''(x) .* (A lam) + 2 qw'lam all run on the
    device, so `optimize` keeps the fused projected-CG path and nothing n-sized crosses PCIe in the loop."""

    def __init__(self, ctx: Context, cons, kind: int, a, c=0.0, xl=None, xu=None, n_global: Optional[int] = None):
        n, m = cons.Jct.n, cons.m_lin
        assert not cons.has_ball and cons.Jct.m == m
        self.ctx, self.n, self.m, self.xc = ctx, n, m, 0.0
        self.p = self.ploc = 0
        self.N, self.M = n, m
        self.Jct, self.R2, self.cons = cons.Jct, 0.0, cons
        self.xl = None if xl is None else np.asarray(xl, dtype=np.float64)
        self.xu = None if xu is None else np.asarray(xu, dtype=np.float64)
        self.n_global = n if n_global is None else n_global
        self.is_diagonal = True
        self.kind = int(kind)
        self.a_dev = None if np.isscalar(a) else ctx.vector(n, np.asarray(a, dtype=np.float64))
        self.c_dev = None if np.isscalar(c) else ctx.vector(n, np.asarray(c, dtype=np.float64))
        self.a0 = float(a) if np.isscalar(a) else 0.0
        self.c0 = float(c) if np.isscalar(c) else 0.0

    def diag_(self, hx: DeviceVector, x: DeviceVector, lam: np.ndarray):
        self._sep(2, x, hx)
        self.cons.hess_diag_(hx, x, lam)


# ------------------------------------------------------------------------------------------------
@dataclass
class Derivatives:
    """Analytic derivatives in the user's variables (the reference gets them by AD,
    src/autodiff_generators.jl -- out of scope).  All callables take HOST arrays."""
    grad_: Callable
    hess_lag_vec_: Optional[Callable]
    jac_c_: Optional[Callable] = None
    jac_d_: Optional[Callable] = None
    # a sparse Lagrangian Hessian on a fixed pattern (:class:`SparseLagrangianHessian`): ``hess_pattern = (rows, cols)`` with
    # ``hess_values_(vals, x, lam)``; ``hess_lag_vec_`` may then be None
    hess_pattern: Optional[tuple] = None
    hess_values_: Optional[Callable] = None


class SparseLagrangianHessian:
    """The structure / values interface for the Lagrangian Hessian (Ipopt's ``eval_h``, JuMP, CasADi): the triplet pattern ``(rows, cols)``
    (0-based host arrays) is declared ONCE; ``values_(vals, x, lam)`` fills the host array ``vals`` of ``nnz`` entries with the triplet values of
    the Hessian of the Lagrangian at the host arrays ``(x, lam)`` -- lam's sign as in the reference's ``hess_lag_vec!(dest, src, x, lam)``:
    dest = (hess f(x) + sum_k lam_k hess c_k(x)) src.  Triangle convention of :class:`SparseHessian`: a triplet with rows != cols counts for
    A_ij AND A_ji (a caller holding a full symmetric matrix passes one triangle), (j, i) is a duplicate of (i, j), duplicates add up in the order
    given; triplets with rows == cols form the diagonal.  At most 32 distinct neighbours per row: more raises the library's error.

    Accepted as ``hess_lag_vec!`` by the 9-argument ``optimize`` and through ``Derivatives(..., hess_pattern=, hess_values_=)``: before every
    truncated-Newton solve ``values_`` is called ONCE, the values are uploaded and placed into a :class:`SparseHessian` and the Hessian diagonal by
    one device call (lfpsqp_sphess_set_values), and the solve runs a :class:`SparseOperator` -- on lfpsqp_projcg_sparse, or with
    ``ctx.options.tridiagonal_one_pass = False`` on the device callback path over lfpsqp_sphess_mul -- with nothing n-sized crossing PCIe inside
    it.  Non-finite values raise ValueError."""

    def __init__(self, rows, cols, values_):
        self.rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).ravel())
        self.cols = np.ascontiguousarray(np.asarray(cols, dtype=np.int64).ravel())
        if self.rows.shape != self.cols.shape:
            raise ValueError("SparseLagrangianHessian: rows and cols of the same length")
        if not callable(values_):
            raise TypeError("SparseLagrangianHessian: values_(vals, x, lam) must be callable")
        self.values_ = values_
        self.nnz = int(self.rows.size)


class _SparsePatternHessian:
    """A :class:`SparseLagrangianHessian` in the protocol ``optimize_core`` knows: ``diag_(hx, x, lam)`` next to ``sparse_hessian``.  ``n`` rows
    on the device (slack rows included: they have no triplets, so their diagonal is 0); ``values_`` sees the first ``nx`` entries of x.
    ``host_values`` tells the driver that ``diag_`` costs a host call: it is not made on an outer iteration already known to be the last."""

    host_values = True

    def __init__(self, ctx, n, nx, hess):
        from .projcg import SparseHessian
        if hess.nnz and (min(hess.rows.min(), hess.cols.min()) < 0 or max(hess.rows.max(), hess.cols.max()) >= nx):
            raise ValueError("SparseLagrangianHessian: a triplet outside the variables")
        self.n, self.nx, self.values_ = n, nx, hess.values_
        self.sparse_hessian, self.pattern = SparseHessian.from_pattern(ctx, n, hess.rows, hess.cols)
        self.vals = np.zeros(hess.nnz)

    def diag_(self, hx: DeviceVector, x: DeviceVector, lam: np.ndarray):
        self.values_(self.vals, x.download(self.nx, 0), lam)
        if not np.all(np.isfinite(self.vals)):
            raise ValueError("SparseLagrangianHessian: values_ produced a non-finite value")
        self.pattern.set_values(self.vals, diag=hx, out=self.sparse_hessian)

    def close(self):
        self.pattern.close()
        self.sparse_hessian.close()


def _hessian_of(dv):
    """What a Derivatives object says about the Lagrangian Hessian: the pattern form when given, else the matrix-free callable."""
    if dv.hess_pattern is None and dv.hess_values_ is None:
        return dv.hess_lag_vec_
    if dv.hess_pattern is None or dv.hess_values_ is None or len(dv.hess_pattern) != 2:
        raise ValueError("Derivatives: hess_pattern = (rows, cols) goes with hess_values_")
    return SparseLagrangianHessian(dv.hess_pattern[0], dv.hess_pattern[1], dv.hess_values_)


def optimize(*args, derivatives: Optional[Derivatives] = None, ctx: Optional[Context] = None, trace=None):
    """optimize(f, x0) / (f, c!, x0, m) / (f, c!, x0, xl, xu, m) / (f, c!, d!, x0, xl, xu, m, p) /
    (f, c!, d!, dl, du, x0, xl, xu, m, p) / (f, grad!, c!, jac!, hess_lag_vec!, x0, xl, xu, m) with an
    optional trailing LFPSQPParams -- host callables, device hot path (projcg!, retractions, tangent
    setup run on the GPU; every user call costs one n-vector PCIe round trip)."""
    args = list(args)
    param = LFPSQPParams()
    if args and isinstance(args[-1], LFPSQPParams):
        param = args.pop()
    if ctx is None:
        ctx = Context(0)
    k = len(args)
    if k == 9:
        f, grad_, c_, jac_, hlv_, x0, xl, xu, m = args
        return _host_core(ctx, f, grad_, c_, jac_, hlv_, x0, xl, xu, m, param, trace)
    if derivatives is None:
        raise NotImplementedError("the AD generators (src/autodiff_generators.jl) are out of scope; pass derivatives=Derivatives(...)")
    dv = derivatives
    if k == 2:
        f, x0 = args
        return _host_core(ctx, f, dv.grad_, None, None, _hessian_of(dv), x0, None, None, 0, param, trace)
    if k == 4:
        f, c_, x0, m = args
        return _host_core(ctx, f, dv.grad_, c_, dv.jac_c_, _hessian_of(dv), x0, None, None, m, param, trace)
    if k == 6:
        f, c_, x0, xl, xu, m = args
        return _host_core(ctx, f, dv.grad_, c_, dv.jac_c_ if m > 0 else None, _hessian_of(dv), x0, xl, xu, m, param, trace)
    if k == 8:      # (f, c!, d!, x0, xl, xu, m, p)   d <= 0                         src/optimize.jl:83
        f, c_, d_, x0, xl, xu, m, p = args
        return _host_slack(ctx, f, c_, d_, -np.inf * np.ones(p), np.zeros(p), x0, xl, xu, m, p, param, dv, trace)
    if k == 10:     # (f, c!, d!, dl, du, x0, xl, xu, m, p)                          src/optimize.jl:13
        f, c_, d_, dl, du, x0, xl, xu, m, p = args
        return _host_slack(ctx, f, c_, d_, dl, du, x0, xl, xu, m, p, param, dv, trace)
    raise TypeError(f"no optimize method with {k} positional arguments")


def _host_slack(ctx, f, c_, d_, dl, du, x0, xl, xu, m, p, param, dv, trace):
    """src/optimize.jl:13-71: slack variables turn dl <= d(x) <= du into equalities d(x) - s = 0 with bounds on
    s; n -> n+p, m -> m+p; the result is truncated to the user's n (:68)."""
    if d_ is None or p == 0:
        return optimize(f, c_, x0, xl, xu, m, param, derivatives=dv, ctx=ctx, trace=trace)
    if not (len(dl) == len(du) == p):
        raise ValueError("Bound vectors dl and du must be of size p")
    x0 = np.asarray(x0, dtype=np.float64)
    n = len(x0)
    xl = -np.inf * np.ones(n) if xl is None else np.asarray(xl, dtype=np.float64)
    xu = np.inf * np.ones(n) if xu is None else np.asarray(xu, dtype=np.float64)
    x0_aux = np.empty(n + p)
    x0_aux[:n] = x0
    d_(x0_aux[n:], x0)
    xl_aux, xu_aux = np.concatenate([xl, dl]), np.concatenate([xu, du])

    def f_aux(x):
        return f(x[:n])

    def c_aux_(cval, x):
        if m > 0:
            c_(cval[:m], x[:n])
        d_(cval[m:m + p], x[:n])
        cval[m:m + p] -= x[n:n + p]
        return cval

    def grad_aux_(g, x):
        dv.grad_(g[:n], x[:n])
        g[n:] = 0.0

    def jac_aux_(J, cval, x):
        J[:, :] = 0.0
        if m > 0:
            dv.jac_c_(J[:m, :n], cval[:m], x[:n])
        dv.jac_d_(J[m:m + p, :n], cval[m:m + p], x[:n])
        cval[m:m + p] -= x[n:n + p]
        J[m:m + p, n:n + p] = -np.eye(p)

    hess = _hessian_of(dv)
    if isinstance(hess, SparseLagrangianHessian):    # the same pattern over n + p rows (the slack rows have no triplets); values_ sees x[:n]
        hlv_aux_ = hess
    else:
        def hlv_aux_(dest, src, x, lam):
            hess(dest[:n], src[:n], x[:n], lam)
            dest[n:] = 0.0

    x, obj, lam, ti = _host_core(ctx, f_aux, grad_aux_, c_aux_, jac_aux_, hlv_aux_, x0_aux, xl_aux, xu_aux, m + p, param, trace, nx=n)
    return x[:n], obj, lam, ti


def _host_core(ctx, f, grad_, c_, jac_, hlv_, x0, xl, xu, m, param, trace, nx=None):
    """Adapters: host callables -> the device-vector contract of optimize_core (no bounds + general
    Hessian: generic projcg path; a :class:`SparseLagrangianHessian`: a SparseOperator refreshed on the device, ``nx`` the variables its
    ``values_`` sees when slack rows follow them)."""
    x0 = np.asarray(x0, dtype=np.float64)
    n = len(x0)

    def f_dev(x):
        return float(f(x.download(n, 0)))

    def grad_dev(g, x):
        gh = np.zeros(n)
        grad_(gh, x.download(n, 0))
        g.upload(gh, 0)

    def jac_dev(Jct, cval, x):
        J = np.zeros((m, n), order='F')
        jac_(J, cval, x.download(n, 0))
        Jct.upload(np.asfortranarray(J.T))

    def hlv_dev(dest, src, x, lam):
        out = np.zeros(n)
        hlv_(out, src.download(n, 0), x.download(n, 0), lam.download(max(m, 1))[:m])
        dest.upload(out, 0)

    if isinstance(hlv_, SparseLagrangianHessian):
        hess = _SparsePatternHessian(ctx, n, n if nx is None else nx, hlv_)
        try:
            return optimize_core(f_dev, grad_dev, c_, jac_dev if m > 0 else None, hess, x0, xl, xu, m, param, ctx=ctx, trace=trace)
        finally:
            hess.close()
    return optimize_core(f_dev, grad_dev, c_, jac_dev if m > 0 else None, hlv_dev, x0, xl, xu, m, param, ctx=ctx, trace=trace)
