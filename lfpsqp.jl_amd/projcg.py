"""projcg! (reference src/projcg.jl) on the device.

``projcg_(x, lam, A, U, b, c, tol=, maxit=, work=)`` keeps the reference's signature and
return value ``(i, nr)`` and, like Julia's method dispatch, picks an implementation
from the operator types:

  * ``A`` a :class:`DiagOperator` and ``U`` a :class:`DeviceBasis`  -> one C call
    (``lfpsqp_projcg``): the fused three-kernel iteration, scalars on the device;
  * anything else supporting the ``mul_`` protocol -> the generic loop below, the
    reference's statement order on device vectors with the BLAS-1/2 primitives
    (what a Julia host gets by defining ``mul!`` on device arrays).
"""
from __future__ import annotations

import ctypes as C
import math

from . import _capi
from .device import (Context, DeviceMatrix, DeviceVector, axpby, dot, gemv_n, gemv_t, nrm2, vmul, waxpby)

WANT_LAMBDA = 1
RESUME = 2
START_GIVEN = 4
START_PROJECTED = 8


class DiagOperator:
    """A = a0*I + diag(dg): device-resident Lagrangian-Hessian action (lfpsqp_diag_op)."""

    def __init__(self, a0: float = 0.0, dg: DeviceVector | None = None):
        self.a0, self.dg = float(a0), dg

    def _c(self):
        return _capi.DiagOp(self.a0, self.dg.h if self.dg is not None else None)

    # mul! protocol (generic path / tests)
    def mul_(self, dest: DeviceVector, v: DeviceVector, a=None, b=None):
        if a is None:
            a, b = 1.0, 0.0
        if self.dg is None:
            return waxpby(a * self.a0, v, b, dest, dest)
        tmp = DeviceVector(dest.ctx, dest.n)
        vmul(self.dg, v, tmp)
        axpby(self.a0, v, 1.0, tmp)
        waxpby(a, tmp, b, dest, dest)
        tmp.free()
        return dest

    def adjoint(self):
        return self


class LowRankOperator:
    """A = a0*I + diag(dg) + V diag(sigma) V' (lfpsqp_lowrank_op): a diagonal Hessian with k <= 8 coupling directions.  On a
    :class:`DeviceBasis` projcg_ runs it on the fused ONE-pass iteration (lfpsqp_projcg_lowrank); the ``mul_`` protocol below is the
    statement-by-statement form (the generic loop / lfpsqp_projcg_op make two passes per iteration with it)."""

    def __init__(self, a0: float, dg: DeviceVector | None, V: DeviceMatrix, k: int | None = None, sigma=None):
        import numpy as np
        self.a0, self.dg, self.V = float(a0), dg, V
        self.k = V.m if k is None else int(k)
        assert 0 <= self.k <= min(V.m, 8)
        self.sigma = None if sigma is None else np.ascontiguousarray(sigma, dtype=np.float64)
        assert self.sigma is None or self.sigma.size >= self.k
        self._t = None

    def _c(self):
        return _capi.LowRankOp(self.a0, self.dg.h if self.dg is not None else None, self.V.h, self.k,
                               self.sigma.ctypes.data if self.sigma is not None else None)

    def mul_(self, dest: DeviceVector, v: DeviceVector, a=None, b=None):
        import numpy as np
        if a is None:
            a, b = 1.0, 0.0
        ctx = dest.ctx
        tmp = DeviceVector(ctx, dest.n)
        if self.dg is not None:
            vmul(self.dg, v, tmp)
            axpby(self.a0, v, 1.0, tmp)
        else:
            waxpby(self.a0, v, 0.0, v, tmp)
        if self.k > 0:
            if self._t is None:
                self._t = DeviceVector(ctx, self.k)
            gemv_t(self.V, v, self._t, self.k)
            if self.sigma is not None:
                self._t.upload(self._t.download(self.k) * self.sigma[:self.k])
            gemv_n(self.V, self._t, tmp, 1.0, 1.0, self.k)
        waxpby(a, tmp, b, dest, dest)
        tmp.free()
        return dest

    def adjoint(self):
        return self


class _CoupledOperator:
    """A = a0*I + diag(dg) + symmetric off-diagonal couplings ``off``: what :class:`TridiagonalOperator`, :class:`BandedOperator`,
    :class:`DiagonalsOperator` and :class:`SparseOperator` share.  A subclass supplies the two C calls: ``_mul`` (the operator on its own) and ``_solve`` (the fused ONE-pass
    projected CG; ``head`` and ``tail`` are the arguments before and after the operator's own).  ``fused = False`` sends projcg_ to the callback
    path (the generic loop / lfpsqp_projcg_op with ``mul_``: two passes over the basis per iteration)."""

    def __init__(self, a0: float, dg: DeviceVector | None, off):
        self.a0, self.dg, self.off = float(a0), dg, off
        self.fused = True
        self._tmp = None

    def _dg_h(self):
        return self.dg.h if self.dg is not None else None

    def mul_(self, dest: DeviceVector, v: DeviceVector, a=None, b=None):
        ctx = dest.ctx
        if a is None:
            ctx.check(self._mul(ctx, v, dest))
            return dest
        if self._tmp is None or self._tmp.n != dest.n:
            self._tmp = DeviceVector(ctx, dest.n)
        ctx.check(self._mul(ctx, v, self._tmp))
        waxpby(a, self._tmp, b, dest, dest)
        return dest

    def adjoint(self):
        return self


class TridiagonalOperator(_CoupledOperator):
    """(A v)_i = (a0 + dg_i) v_i + off_{i-1} v_{i-1} + off_i v_{i+1} (lfpsqp_tridiag_op): a diagonal Hessian plus nearest-neighbour
    couplings.  ``off``: DeviceVector of length n (entry i couples rows i and i+1; the last entry is ignored).  On a :class:`DeviceBasis`
    projcg_ runs it on the fused ONE-pass iteration (lfpsqp_projcg_tridiag); ``mul_`` is the operator on its own (lfpsqp_tridiag_mul), which
    the generic loop / lfpsqp_projcg_op use -- two passes over the basis per iteration.
    With bounds (a stacked basis, :class:`InequalityDecompProject`): ``dg`` is a :class:`StackedVector` (the augmented diagonal, both halves)
    and ``off`` has N entries, the couplings of the x half -- the Newton map blockdiag(T, diag) of src/inequality_helper.jl:144-158, on the same
    one-pass iteration."""

    def __init__(self, a0: float, dg: DeviceVector | None, off: DeviceVector):
        super().__init__(a0, dg, off)

    def _c(self):
        return _capi.TridiagOp(self.a0, self._dg_h(), self.off.h)

    def _mul(self, ctx, v, out):
        a_c = self._c()
        return ctx.L.lfpsqp_tridiag_mul(ctx.h, C.byref(a_c), v.h, out.h)

    def _solve(self, ctx, head, tail):
        a_c = self._c()
        return ctx.L.lfpsqp_projcg_tridiag(*head, C.byref(a_c), *tail)


class BandedOperator(_CoupledOperator):
    """(A v)_i = (a0 + dg_i) v_i + sum_{k=1..bw} (off_k[i-k] v_{i-k} + off_k[i] v_{i+k}), 1 <= bw <= 4: a diagonal Hessian plus couplings up to
    ``bw`` rows apart (second or higher differences: Whittaker / Hodrick-Prescott smoothing, curvature penalties).  ``off``: DeviceMatrix with n
    rows and at least ``bw`` columns, column k-1 = off_k (entry i couples rows i and i+k; entries with i + k >= n are ignored).  On a
    :class:`DeviceBasis` projcg_ runs it on the fused ONE-pass iteration (lfpsqp_projcg_band; bw = 1 is the tridiagonal path, bit for bit);
    ``mul_`` is the operator on its own (lfpsqp_band_mul), which the generic loop / lfpsqp_projcg_op use -- two passes over the basis per
    iteration.  ``fused = False`` sends projcg_ to that callback path.  With bounds (a stacked basis): ``dg`` is a :class:`StackedVector` and
    ``off`` has N rows, the couplings of the x half, as for :class:`TridiagonalOperator`."""

    def __init__(self, a0: float, dg: DeviceVector | None, off: DeviceMatrix, bw: int):
        super().__init__(a0, dg, off)
        self.bw = int(bw)

    def _mul(self, ctx, v, out):
        return ctx.L.lfpsqp_band_mul(ctx.h, self.a0, self._dg_h(), self.off.h, self.bw, v.h, out.h)

    def _solve(self, ctx, head, tail):
        return ctx.L.lfpsqp_projcg_band(*head, self.a0, self._dg_h(), self.off.h, self.bw, *tail)


class DiagonalsOperator(_CoupledOperator):
    """(A v)_i = (a0 + dg_i) v_i + sum_k (off_k[i - s_k] v_{i - s_k} + off_k[i] v_{i + s_k}) for 1 <= K <= 13 off-diagonals at ARBITRARY distances
    ``dists`` = (s_1 < ... < s_K): the Hessian of a smoothness / diffusion term on a 2-D or 3-D field in row-major order ((1, nx), (1, nx, nx ny),
    (1, nx - 1, nx, nx + 1) for the 5-, 7- and 9-point stencils, 13 distances for the 27-point one; a periodic axis adds its wrap-around edges as
    further distances; :func:`lfpsqp_jl_amd.problems.grid_laplacian`, :func:`lfpsqp_jl_amd.problems.graph_diagonals`).  ``off``: DeviceMatrix with
    n rows and at least K columns, column k-1 = off_k (entry i couples rows i and i + s_k; entries with i + s_k >= n are ignored; the ends of a
    grid line are zeros in the data).  On a :class:`DeviceBasis` projcg_ runs it on the fused ONE-pass iteration (lfpsqp_projcg_diags for
    K <= 4, exactly as before; lfpsqp_projcg_stencil for 5 .. 13); ``mul_`` is the operator on its own (lfpsqp_diags_mul / lfpsqp_stencil_mul),
    which the generic loop / lfpsqp_projcg_op use -- two passes over the basis per iteration.  ``fused = False`` sends projcg_ to that callback
    path.  More than 13 distances: ValueError.  With bounds (a stacked basis): ``dg`` is a :class:`StackedVector` and ``off`` has N rows, the
    couplings of the x half, as for :class:`BandedOperator`.

    SET-UP COST.  The one-pass solve forms U'A U first: K + 1 weighted Gram passes over the basis (K + 2 when A is not diagonally dominant), so
    14 or 15 at K = 13, where the callback path has none.  Not measured on the MI355X yet (FINDINGS.md 18): by the figures of the narrow path (a
    run-time-distance Gram pass 4.6-5.1 ms at (1e7, 128), about 1.2 ms gained per iteration) the break-even against ``fused = False`` lies
    at several tens of iterations per solve at K = 13 -- for shorter solves ``fused = False`` is the better choice;
    ``tools/time_diags.py GRID M --corners --split-callback`` measures both for a given shape."""

    MAX_DIAGS = 13                                  # LFPSQP_STENCIL_MAX_DIAGS

    def __init__(self, a0: float, dg: DeviceVector | None, off: DeviceMatrix, dists):
        super().__init__(a0, dg, off)
        self.dists = tuple(int(s) for s in dists)
        if len(self.dists) > self.MAX_DIAGS:
            raise ValueError(f"DiagonalsOperator: {len(self.dists)} off-diagonals, at most {self.MAX_DIAGS}")
        self._dist_c = (_capi.c_i64 * max(len(self.dists), 1))(*self.dists)
        self._wide = len(self.dists) > 4            # (up to four distances: the entries and kernels of the narrow descriptor)

    def _mul(self, ctx, v, out):
        mul = ctx.L.lfpsqp_stencil_mul if self._wide else ctx.L.lfpsqp_diags_mul
        return mul(ctx.h, self.a0, self._dg_h(), self.off.h, len(self.dists), self._dist_c, v.h, out.h)

    def _solve(self, ctx, head, tail):
        solve = ctx.L.lfpsqp_projcg_stencil if self._wide else ctx.L.lfpsqp_projcg_diags
        return solve(*head, self.a0, self._dg_h(), self.off.h, len(self.dists), self._dist_c, *tail)


def _triplets(who: str, names: str, i, j, w=None):
    """The index lists of an edge / triplet list as contiguous int64 arrays of one length, with ``w`` (a scalar or one value per entry) as a
    contiguous float64 array of that length."""
    import numpy as np
    ii = np.ascontiguousarray(np.asarray(i, dtype=np.int64).ravel())
    jj = np.ascontiguousarray(np.asarray(j, dtype=np.int64).ravel())
    if ii.shape != jj.shape:
        raise ValueError(f"{who}: {names} of the same length")
    return ii, jj, None if w is None else np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.float64), ii.shape))


class SparseHessian:
    """The symmetric off-diagonal part S of a sparse Hessian A = a0*I + diag(dg) + S as a device handle (lfpsqp_sphess): built ONCE from the
    undirected edge list ``(i, j, w)`` (0-based host arrays in any order, ``w`` a scalar or one value per edge: the entry A_ij = A_ji; duplicates
    and mirrored duplicates add up), at most 32 entries per row.  The values stay as built unless the handle is the ``out`` of :meth:`edge_eval`, which rewrites them on the device (a
    handle made by :meth:`like`: the same pattern, its own values).  ``n``, ``nedges`` (distinct
    undirected edges), ``row_width`` (the largest row degree) and ``edge_width`` (the most edges one row owns: the number of set-up passes of a
    one-pass solve) describe what was built.  The diagonal is not part of it: i == j raises."""

    def __init__(self, ctx: Context, n: int, i, j, w):
        ii, jj, ww = _triplets("SparseHessian", "i and j", i, j, w)
        self._open(ctx, ctx.L.lfpsqp_sphess_create, int(n), ii.size, ii.ctypes.data, jj.ctypes.data, ww.ctypes.data)

    def _open(self, ctx, create, *args):
        """This object as the wrapper of the handle that ``create(ctx.h, *args, &h)`` makes."""
        self.ctx, self.h = ctx, None
        h = C.c_void_p()
        ctx.check(create(ctx.h, *args, C.byref(h)))
        self.h = h
        out = [_capi.c_i64() for _ in range(6)]
        ctx.check(ctx.L.lfpsqp_sphess_info(self.h, *(C.byref(o) for o in out[:4])))
        ctx.check(ctx.L.lfpsqp_sphess_points_info(self.h, *(C.byref(o) for o in out[4:])))
        self.n, self.nedges, self.row_width, self.edge_width, self.npoints, self.dim = (o.value for o in out)
        return self

    @classmethod
    def from_points(cls, ctx: Context, n: int, npoints: int, dim: int, pi, pj, w) -> "SparseHessian":
        """The handle of a PAIR term between ``npoints`` points of ``dim`` = 2 or 3 unknowns each, interleaved (unknown ``dim*p + c`` is component
        c of point p; lfpsqp_sphess_create_points): ``(pi, pj, w)`` are undirected edges between points (0-based, any order, ``w`` a scalar or one
        weight per edge; duplicates add up), every edge a dense dim x dim block of entries holding w, every point the entries between its own
        components holding 0.0.  ``n`` >= dim*npoints rows; the rows behind the points (a slack row) carry no couplings.  At most 15 neighbours
        per point in 2-D and 10 in 3-D (32 entries per scalar row).  ``npoints`` and ``dim`` are kept (0 for every other handle; :meth:`like`
        copies them); :meth:`pair_eval` evaluates the term."""
        ii, jj, ww = _triplets("SparseHessian.from_points", "pi and pj", pi, pj, w)
        return object.__new__(cls)._open(ctx, ctx.L.lfpsqp_sphess_create_points, int(n), int(npoints), int(dim), ii.size, ii.ctypes.data, jj.ctypes.data,
                                         ww.ctypes.data)

    def like(self) -> "SparseHessian":
        """A second handle on the same pattern (lfpsqp_sphess_like): the index arrays are shared, the values are its own, initialised to this
        handle's.  The two may be closed in either order."""
        return object.__new__(SparseHessian)._open(self.ctx, self.ctx.L.lfpsqp_sphess_like, self.h)

    def _eval(self, entry: str, kind, delta, scale, x, grad, diag, out, want_f):
        """lfpsqp_sphess_<entry>: what :meth:`edge_eval` and :meth:`pair_eval` document."""
        ctx = self.ctx
        if out is not None and out.ctx is not ctx:
            raise ValueError(f"SparseHessian.{entry}: the output handle belongs to another context")
        f = C.c_double()
        ctx.check(getattr(ctx.L, "lfpsqp_sphess_" + entry)(ctx.h, self.h, int(kind), float(delta), float(scale), x.h, C.byref(f) if want_f else None,
                                                           grad.h if grad is not None else None, diag.h if diag is not None else None,
                                                           out.h if out is not None else None))
        return f.value if want_f else None

    def edge_eval(self, kind: int, delta: float, scale: float, x, grad=None, diag=None, out=None, want_f: bool = True):
        """The edge term scale * sum_e w_e psi(x_i - x_j) with this handle's values as the weights w_e (lfpsqp_sphess_edge_eval; ``kind`` 0:
        t^2/2, 1: t^2/2 + t^4/4, 2: pseudo-Huber with scale ``delta``): returns its value (None with ``want_f=False``: no reduction is run),
        ADDS its gradient to ``grad`` and scale * sum_j w_ij psi'' to ``diag`` (the first ``n`` entries of either; ``x`` may be longer, a stacked
        iterate: its first ``n`` entries are read) and writes the off-diagonal values -(scale w_e) psi'' into ``out``, a handle made by
        :meth:`like`.  With nothing but the value asked for, the kernel writes no vector.  This handle is never modified."""
        return self._eval("edge_eval", kind, delta, scale, x, grad, diag, out, want_f)

    def point_values(self, pi, pj, vals) -> "SparseHessian":
        """A handle on this pattern holding one PARAMETER per point edge (lfpsqp_sphess_points_values): ``vals[e]`` -- a rest length, a measured
        distance; finite and >= 0 -- on all dim^2 entries of the point edge ``(pi[e], pj[e])`` and 0.0 inside a point: the ``params`` of
        :meth:`pair_eval`.  The list must name every point edge of this handle (made by :meth:`from_points`, or a handle on its pattern) exactly
        once, in any order and either orientation: a parameter does not add up, so a duplicate, a foreign edge or a missing one is refused."""
        ii, jj, vv = _triplets("SparseHessian.point_values", "pi and pj", pi, pj, vals)
        return object.__new__(SparseHessian)._open(self.ctx, self.ctx.L.lfpsqp_sphess_points_values, self.h, ii.size, ii.ctypes.data, jj.ctypes.data,
                                                   vv.ctypes.data)

    def _pair_eval_ex(self, kind, delta, params, anchors, scale, x, grad, diag, out, want_f):
        ctx = self.ctx
        for name, o in (("output handle", out), ("parameter handle", params), ("anchors", anchors)):
            if o is not None and o.ctx is not ctx:
                raise ValueError(f"SparseHessian.pair_eval: the {name} belongs to another context")
        f = C.c_double()
        h = lambda o: o.h if o is not None else None
        ctx.check(ctx.L.lfpsqp_sphess_pair_eval_ex(ctx.h, self.h, int(kind), float(delta), h(params), h(anchors), float(scale), x.h,
                                                   C.byref(f) if want_f else None, h(grad), h(diag), h(out)))
        return f.value if want_f else None

    def pair_eval(self, kind: int, delta: float, scale: float, x, grad=None, diag=None, out=None, want_f: bool = True, params=None, anchors=None):
        """The pair term scale * sum_e w_e psi(x_p - x_q) between the points of a handle made by :meth:`from_points`, with this handle's values as
        the weights (lfpsqp_sphess_pair_eval; t = x_p - x_q in R^dim, ``kind`` 0: |t|^2/2, 1: (|t| - delta)^2/2, a spring of rest length
        ``delta``, 2: the radial pseudo-Huber function delta^2 (sqrt(1 + |t|^2/delta^2) - 1)).  The conventions are those of :meth:`edge_eval`:
        the value is returned (None with ``want_f=False``), the gradient is ADDED to ``grad`` and the Hessian's diagonal to ``diag`` (their first
        dim*npoints entries; ``x`` may be longer), and ``out``, a handle made by :meth:`like`, receives the off-diagonal entries: the dim x dim
        block -(scale w)(a I + b t t') per edge and the entries between a point's own components.  This handle is never modified.  Kind 1 with
        two coincident points joined by an edge is a singularity of the potential: the outputs are then not finite.
        ``params`` (a handle made by :meth:`point_values`): one rest length (kind 1) or one delta (kind 2) per edge instead of ``delta``; kind 0 has
        no parameter and refuses it.  ``anchors`` (a :class:`PointAnchors` made for this handle) adds scale * sum_k u_k psi(x_p - a_k; par_k): to
        the value, the gradient, the diagonal and the entries between a point's own components; no entry between points changes.  With either
        the call is lfpsqp_sphess_pair_eval_ex, and ``delta`` is checked only where it is used (no ``params``, or anchors without ``par``)."""
        if params is not None or anchors is not None:
            return self._pair_eval_ex(kind, delta, params, anchors, scale, x, grad, diag, out, want_f)
        return self._eval("pair_eval", kind, delta, scale, x, grad, diag, out, want_f)

    @classmethod
    def from_pattern(cls, ctx: Context, n: int, rows, cols):
        """``(S, pattern)`` for the structure / values interface: ``S`` a handle over the off-diagonal triplets of ``(rows, cols)`` (0-based, the
        edge-list convention of the constructor; triplets with rows == cols are dropped for the handle) created with zero values, and
        ``pattern`` the :class:`SparsePattern` over the FULL triplet list, diagonal included, whose :meth:`SparsePattern.set_values` fills ``S`` (or
        any handle made by :meth:`like`) and a diagonal vector from ``nnz`` values."""
        rr, cc, _ = _triplets("SparseHessian.from_pattern", "rows and cols", rows, cols)
        off = rr != cc
        S = cls(ctx, n, rr[off], cc[off], 0.0)
        try:
            return S, SparsePattern(S, rr, cc)
        except Exception:
            S.close()
            raise

    def close(self):
        if self.h is not None:
            self.ctx.L.lfpsqp_sphess_free(self.ctx.h, self.h)
            self.h = None

    free = close

    def __del__(self):
        try:
            if getattr(self.ctx, "h", None) is not None:
                self.close()
        except Exception:
            pass


class PointAnchors:
    """Fixed points that points of ``W`` (a :class:`SparseHessian` made by :meth:`SparseHessian.from_points`, or a handle on its pattern) are tied
    to (lfpsqp_anchors): anchor k ties point ``point[k]`` to the position ``pos[k]`` (nanchors x dim) with the weight ``u[k]`` (a scalar or one
    per anchor) and the parameter ``par[k]`` -- the distance to keep from the anchor under kind 1 (0: a pin), the delta of kind 2; ``None``: the
    ``delta`` of the call.  The supports of a truss, the beacons of a localisation problem: soft terms u_k psi(x_p - a_k; par_k), evaluated by
    :meth:`SparseHessian.pair_eval` with ``anchors=`` this object.  At most 8 anchors on one point; ``nanchors`` and ``width`` (the most anchors
    on one point) describe what was built.  The object keeps ``W``'s (n, npoints, dim), not ``W``: it may outlive it, and serves any handle with
    those numbers."""

    def __init__(self, W: SparseHessian, point, pos, u, par=None):
        import numpy as np
        self.ctx = ctx = W.ctx
        self.h = None
        pt = np.ascontiguousarray(np.asarray(point, dtype=np.int64).ravel())
        ph = np.ascontiguousarray(np.asarray(pos, dtype=np.float64).reshape(pt.size, -1))
        if ph.shape[1] != W.dim:
            raise ValueError(f"PointAnchors: pos has {ph.shape[1]} columns for points of {W.dim} unknowns")
        uh = np.ascontiguousarray(np.broadcast_to(np.asarray(u, dtype=np.float64), pt.shape))
        rh = None if par is None else np.ascontiguousarray(np.broadcast_to(np.asarray(par, dtype=np.float64), pt.shape))
        h = C.c_void_p()
        ctx.check(ctx.L.lfpsqp_anchors_create(ctx.h, W.h, pt.size, pt.ctypes.data, ph.ctypes.data, uh.ctypes.data, None if rh is None else rh.ctypes.data,
                                              C.byref(h)))
        self.h = h
        out = [_capi.c_i64() for _ in range(2)]
        ctx.check(ctx.L.lfpsqp_anchors_info(self.h, *(C.byref(o) for o in out)))
        self.nanchors, self.width = (o.value for o in out)

    def close(self):
        if self.h is not None:
            self.ctx.L.lfpsqp_anchors_free(self.ctx.h, self.h)
            self.h = None

    free = close

    def __del__(self):
        try:
            if getattr(self.ctx, "h", None) is not None:
                self.close()
        except Exception:
            pass


class SparsePattern:
    """A triplet pattern ``(rows, cols)`` declared ONCE against the pattern of a :class:`SparseHessian` ``S`` (lfpsqp_sphess_map): the convention is
    the constructor's -- a triplet counts for A_ij and A_ji, duplicates and mirrored duplicates add up in the order given -- and rows == cols is
    allowed: those triplets form the diagonal.  Every off-diagonal triplet must be an edge of ``S`` (the library's error names the entry).  ``nnz``,
    ``ndiag`` (triplets on the diagonal) and ``max_dup`` (the longest chain of duplicates) describe what was declared.  The map holds a reference
    on the pattern: it and the handles may be closed in any order."""

    def __init__(self, S: SparseHessian, rows, cols):
        self.ctx = ctx = S.ctx
        self.h = None
        self._vals = None
        rr, cc, _ = _triplets("SparsePattern", "rows and cols", rows, cols)
        h = C.c_void_p()
        ctx.check(ctx.L.lfpsqp_sphess_map_create(ctx.h, S.h, rr.size, rr.ctypes.data, cc.ctypes.data, C.byref(h)))
        self.h = h
        out = [_capi.c_i64() for _ in range(3)]
        ctx.check(ctx.L.lfpsqp_sphess_map_info(self.h, *(C.byref(o) for o in out)))
        self.nnz, self.ndiag, self.max_dup = (o.value for o in out)

    def set_values(self, vals, diag=None, out=None):
        """``vals`` -- a :class:`DeviceVector` of at least ``nnz`` entries, or a host array, uploaded into a vector this object keeps -- placed into
        both forms of ``out`` (any handle on the pattern) and into ``diag`` (lfpsqp_sphess_set_values): a stored value is the sum of its triplets in
        the order given, the bits :class:`SparseHessian` builds from the same triplets; the first ``n`` entries of ``diag`` are OVERWRITTEN with the
        sums of the diagonal triplets (0 where a row has none), entries behind them are left alone.  Values are not checked for finiteness."""
        ctx = self.ctx
        if out is not None and out.ctx is not ctx:
            raise ValueError("SparsePattern.set_values: the output handle belongs to another context")
        if not isinstance(vals, DeviceVector):
            import numpy as np
            vh = np.ascontiguousarray(np.asarray(vals, dtype=np.float64).ravel())
            if vh.size < self.nnz:
                raise ValueError(f"SparsePattern.set_values: {vh.size} values for {self.nnz} triplets")
            if self._vals is None:
                self._vals = DeviceVector(ctx, max(self.nnz, 1))
            if self.nnz > 0:
                self._vals.upload(vh[:self.nnz])
            vals = self._vals
        ctx.check(ctx.L.lfpsqp_sphess_set_values(ctx.h, self.h, vals.h, diag.h if diag is not None else None, out.h if out is not None else None))

    def close(self):
        if self.h is not None:
            self.ctx.L.lfpsqp_sphess_map_free(self.ctx.h, self.h)
            self.h = None
        if self._vals is not None:
            self._vals.free()
            self._vals = None

    free = close

    def __del__(self):
        try:
            if getattr(self.ctx, "h", None) is not None:
                self.close()
        except Exception:
            pass


class SparseOperator(_CoupledOperator):
    """(A v)_i = (a0 + dg_i) v_i + sum_{j in row i of S} S_ij v_j for a :class:`SparseHessian` ``S``: a diagonal Hessian plus couplings described by
    ROW INDICES -- a smoothness term on a triangle mesh, a k-nearest-neighbour graph, a grid in any numbering, the 26-neighbour periodic 3-D stencil:
    everything :class:`DiagonalsOperator` cannot express (more than 13 distinct distances j - i).  On a :class:`DeviceBasis` projcg_ runs it on the
    fused ONE-pass iteration (lfpsqp_projcg_sparse); ``mul_`` is the operator on its own (lfpsqp_sphess_mul), which the generic loop /
    lfpsqp_projcg_op use -- two passes over the basis per iteration.  ``fused = False`` sends projcg_ to that callback path.  With bounds (a stacked
    basis): ``dg`` is a :class:`StackedVector` and ``S`` has N rows, the couplings of the x half, as for :class:`DiagonalsOperator`.

    SET-UP COST.  The one-pass solve forms U'A U first: ``S.edge_width`` + 1 weighted Gram passes over the basis (+ 2 when A is not diagonally
    dominant) whose operand gathers the partner rows, where the callback path has none; per iteration its two vector kernels move 12 bytes per
    stored entry where the distance form moves 8 bytes per two.  Measured at (1e7, 128) on one MI355X (FINDINGS.md 19; ms per
    iteration / set-up per solve): the 27-point stencil of 216^3 (row_width 26, edge_width 13) 3.92 / 79 against 4.27 / 4.4 on the callback
    path -- break-even at 214 iterations per solve -- and 3.63 / 79 for :class:`DiagonalsOperator` on the same edges, which stays the form for
    any graph with at most 13 distances; a triangulated 3200 x 3125 grid in row-major numbering (row_width 6, edge_width 3) 2.36 / 23 against
    3.57 / 3.6, break-even at 16 iterations; the SAME mesh in a permuted numbering 5.28 / 101 against 4.51 / 4.7: without locality every
    gathered value is a cache line of its own and the one-pass form LOSES per iteration and in the set-up -- use ``fused = False`` for a graph
    whose numbering has no locality (and for short solves at large row_width).  ``tools/time_sphess.py GRID M [--corners | --mesh [--permute]]``
    measures both paths for a given graph and says where the one-pass form never pays."""

    def __init__(self, a0: float, dg: DeviceVector | None, S: SparseHessian):
        if dg is not None and dg.ctx is not S.ctx:
            raise ValueError("SparseOperator: the handle belongs to another context")
        super().__init__(a0, dg, None)
        self.S = S

    def _check(self, ctx):
        if ctx is not self.S.ctx:
            raise ValueError("SparseOperator: the handle belongs to another context")

    def _mul(self, ctx, v, out):
        self._check(ctx)
        return ctx.L.lfpsqp_sphess_mul(ctx.h, self.a0, self._dg_h(), self.S.h, v.h, out.h)

    def _solve(self, ctx, head, tail):
        self._check(ctx)
        return ctx.L.lfpsqp_projcg_sparse(*head, self.a0, self._dg_h(), self.S.h, *tail)


class DeviceBasis:
    """Orthonormal U = Z[:, :ncols] (``view(U, :, 1:rank)``, src/optimize.jl:370).
    ``Z = None`` with ``generator = (A, W)``: the basis in FACTORED form U = A W -- never materialised; projcg_, the Newton retraction and
    the projections stream A and apply the small factor W on the side (lfpsqp_basis.Z == NULL, FINDINGS.md 5.3)."""

    def __init__(self, Z: DeviceMatrix | None, ncols: int | None = None, generator=None, sparse=None):
        self.Z = Z
        assert Z is not None or generator is not None
        self.ncols = (Z.m if Z is not None else generator[1].shape[1]) if ncols is None else int(ncols)
        self.generator = generator          # optional (A, W) with Z == A @ W (ksvd_'s W): lfpsqp_basis.A / .W
        self.sparse = sparse                # optional SparseMatrix twin of A's leading columns: projcg_ runs on the nonzeros (lfpsqp_basis.SA)

    @property
    def ctx(self):
        return self.Z.ctx if self.Z is not None else self.generator[0].ctx

    def _c(self):
        zh = self.Z.h if self.Z is not None else None
        if self.generator is not None:
            A, W = self.generator
            return _capi.Basis(zh, self.ncols, None, None, None, None, A.h, W.ctypes.data, None,
                               self.sparse.h if self.sparse is not None else None)
        return _capi.Basis(zh, self.ncols, None, None, None, None)

    def _factored(self):
        return self.generator is not None and (self.sparse is not None or self.Z is None)

    def mul_(self, dest, v, a=None, b=None):
        if a is None:
            a, b = 1.0, 0.0
        if self._factored():                # U t = A (W t): on the nonzeros (lfpsqp_basis.SA) or over the dense generator (Z == NULL)
            c = self.ctx
            bs = self._c()
            c.check(c.L.lfpsqp_q_gemv_n(c.h, C.byref(bs), float(a), None, v.h, float(b), dest.h))
            return dest
        return gemv_n(self.Z, v, dest, a, b, self.ncols)

    def adjoint(self):
        return _BasisAdjoint(self)


class _BasisAdjoint:
    def __init__(self, basis):
        self.basis = basis

    def mul_(self, dest, v, a=None, b=None):
        assert a is None
        if self.basis._factored():          # U'v = W'(A'v)
            c = self.basis.ctx
            bs = self.basis._c()
            c.check(c.L.lfpsqp_q_gemv_t(c.h, C.byref(bs), v.h, None, dest.h))
            return dest
        return gemv_t(self.basis.Z, v, dest, self.basis.ncols)

    def adjoint(self):
        return self.basis


class ProjCGWork:
    """ProjCGWork(n, m) (src/projcg.jl:1-11); only g, d, rp, Utr exist on the device."""

    def __init__(self, ctx: Context, n: int, m: int, stacked_N: int | None = None, against=None, extra: int = 0):
        """n = length of the n-vectors on this rank; with bounds pass stacked_N = N and the
        vectors get the stacked [x | gap | y] layout (length hs + N).
        ``against`` (DeviceMatrix): the basis these vectors will be streamed with -- they then come from one placement-tuned
        allocation (lfpsqp_vecs_alloc_placed, FINDINGS.md 6), together with ``extra`` more vectors of the same kind left in
        ``self.placed_extra`` (in the trial, the first of them plays the operator diagonal: use it for DiagOperator).
        ``against = ("new", rows, m)``: the basis matrix is allocated here as well, jointly with the vectors (every pair of candidate
        allocations tried, lfpsqp_basis_work_alloc_placed), and left in ``self.basis``."""
        self.placed_extra = []
        self.basis = None
        if isinstance(against, tuple):              # ("new", rows, m): allocate the basis too, jointly (lfpsqp_basis_work_alloc_placed) -> self.basis
            self.basis, vs = ctx.basis_and_vectors_placed(against[1], against[2], 3 + extra, stacked_N=stacked_N)
            against = None
            self.g, self.d = vs[0], vs[1]
            self.placed_extra = vs[2:2 + extra]
            self.rp = vs[2 + extra]
        elif against is not None:
            vs = ctx.vectors_placed(against, n, 3 + extra, stacked_N=stacked_N)
            self.g, self.d = vs[0], vs[1]
            self.placed_extra = vs[2:2 + extra]
            self.rp = vs[2 + extra]
        elif stacked_N is not None:
            from .inequality import StackedVector
            self.g, self.d, self.rp = (StackedVector(ctx, stacked_N) for _ in range(3))
        else:
            self.g, self.d, self.rp = (DeviceVector(ctx, n) for _ in range(3))
        # (3 m + 8: room behind the m coefficients for the sums lfpsqp_tangent_step parks for LFPSQP_PROJCG_START_PROJECTED)
        self.Utr = DeviceVector(ctx, 3 * max(m, 1) + 8)
        # extra scratch for a general operator A (lfpsqp_projcg_op's Av) and for the all-Python loop, allocated on demand
        self.Av = None
        self._extra = None

    def _c(self):
        return _capi.ProjCGWorkC(self.g.h, self.d.h, self.rp.h, self.Utr.h)


def projcg_(x: DeviceVector, lam: DeviceVector | None, A, U, b: DeviceVector, c: DeviceVector | None,
            tol: float = 1e-6, maxit: int | None = None, work: ProjCGWork | None = None, n_global: int | None = None,
            want_lambda: bool = True, resume: bool = False, start_given: bool = False, start_projected: bool = False):
    """``resume=True`` (device path only): ``maxit`` MORE iterations of the solve the previous call left at its iteration
    limit (LFPSQP_PROJCG_RESUME); the returned count runs from the start of the solve.
    ``start_given=True`` (device path, factored plain basis, ``c`` None): ``work.rp`` holds r0 = -b and ``work.Utr`` holds U'r0, left there
    by lfpsqp_tangent_step -- the solve skips its own residual pass (LFPSQP_PROJCG_START_GIVEN).
    ``start_projected=True``: the initial projection itself was made by lfpsqp_tangent_step (LFPSQP_TANGENT_INIT_PROJCG): ``work.g``, ``work.d``
    and the sums parked in ``work.Utr`` are the state the first iteration starts from (LFPSQP_PROJCG_START_PROJECTED)."""
    ctx = x.ctx
    n = b.n
    m = U.ncols if hasattr(U, "ncols") else (c.n if c is not None else 0)
    if n_global is None:
        n_global = n
    if maxit is None:
        maxit = n_global + m
    from .inequality import InequalityDecompProject
    stacked = isinstance(U, InequalityDecompProject)
    if stacked and n_global == n:
        n_global = 2 * U.idecomp.N          # the reference's length(b)
    if work is None:
        work = ProjCGWork(ctx, n, m, U.idecomp.N if stacked else None)
    if isinstance(A, DiagOperator) and (isinstance(U, DeviceBasis) or stacked):
        iters = _capi.c_i64()
        nr = C.c_double()
        a_c, u_c, w_c = A._c(), U._c(), work._c()
        flags = ((WANT_LAMBDA if (want_lambda and lam is not None) else 0) | (RESUME if resume else 0) | (START_GIVEN if start_given else 0)
                 | (START_PROJECTED if start_projected else 0))
        ctx.check(ctx.L.lfpsqp_projcg(ctx.h, x.h, lam.h if lam is not None else None, C.byref(a_c), C.byref(u_c), b.h,
                                      c.h if c is not None else None, float(tol), int(maxit), int(n_global), flags,
                                      C.byref(w_c), C.byref(iters), C.byref(nr)))
        return iters.value, nr.value
    if isinstance(A, LowRankOperator) and isinstance(U, DeviceBasis) and not stacked and not (resume or start_given or start_projected) and getattr(A, "fused", True):
        iters = _capi.c_i64()
        nr = C.c_double()
        a_c, u_c, w_c = A._c(), U._c(), work._c()
        flags = WANT_LAMBDA if (want_lambda and lam is not None) else 0
        rc = ctx.L.lfpsqp_projcg_lowrank(ctx.h, x.h, lam.h if lam is not None else None, C.byref(a_c), C.byref(u_c), b.h,
                                         c.h if c is not None else None, float(tol), int(maxit), int(n_global), flags,
                                         C.byref(w_c), C.byref(iters), C.byref(nr))
        if rc != -5:                 # LFPSQP_ERR_UNSUPPORTED (a shape without the one-pass iteration): the callback path below
            ctx.check(rc)
            return iters.value, nr.value
    if isinstance(A, _CoupledOperator) and (isinstance(U, DeviceBasis) or stacked) and not (resume or start_projected) and A.fused:
        if getattr(work, "Av", None) is None:
            work.Av = DeviceVector(ctx, n)
        iters = _capi.c_i64()
        nr = C.c_double()
        u_c, w_c = U._c(), work._c()
        flags = (WANT_LAMBDA if (want_lambda and lam is not None) else 0) | (START_GIVEN if start_given else 0)
        rc = A._solve(ctx, (ctx.h, x.h, lam.h if lam is not None else None),
                      (work.Av.h, C.byref(u_c), b.h, c.h if c is not None else None, float(tol), int(maxit), int(n_global), flags,
                       C.byref(w_c), C.byref(iters), C.byref(nr)))
        if rc != -5 or start_given:  # LFPSQP_ERR_UNSUPPORTED (no one-pass iteration for this shape / more than one rank): the callback path below
            ctx.check(rc)
            return iters.value, nr.value
    if resume or start_given or start_projected:
        raise ValueError("resume / start_given / start_projected are features of the device-resident projcg loop")
    if (isinstance(U, DeviceBasis) or stacked) and hasattr(A, "mul_"):
        # general A (the LinearMap case, src/optimize.jl:228-230) on the C loop: lfpsqp_projcg_op calls back once per iteration
        # for A*d; the products stay on the device and nothing in the loop waits for it (no per-dot host round trips)
        if getattr(work, "Av", None) is None:
            work.Av = work.g.__class__(ctx, work.g.N) if hasattr(work.g, "N") else DeviceVector(ctx, n)
        Av = work.Av
        known = {x.h.value: x, work.d.h.value: work.d}

        def tramp(user, src_h, dst_h):
            try:
                A.mul_(Av, known[src_h])
                return 0
            except Exception as e:       # never unwind through C
                print("operator callback failed:", repr(e))
                return 1
        cb = _capi.OPFUN(tramp)
        iters = _capi.c_i64()
        nr = C.c_double()
        u_c, w_c = U._c(), work._c()
        flags = WANT_LAMBDA if (want_lambda and lam is not None) else 0
        ctx.check(ctx.L.lfpsqp_projcg_op(ctx.h, x.h, lam.h if lam is not None else None, cb, None, Av.h, C.byref(u_c), b.h,
                                         c.h if c is not None else None, float(tol), int(maxit), int(n_global), flags,
                                         C.byref(w_c), C.byref(iters), C.byref(nr)))
        del cb
        return iters.value, nr.value
    return _projcg_generic(x, lam, A, U, b, c, tol, maxit, work, n_global, m)


def _projcg_generic(x, lam, A, U, b, c, tol, maxit, work, n_global, m):
    """src/projcg.jl:55-120 statement by statement on device vectors."""
    ctx = x.ctx
    n = b.n
    if work._extra is None:
        mk = (lambda: g0.__class__(ctx, g0.N)) if hasattr(work.g, "N") else (lambda: DeviceVector(ctx, n))
        g0 = work.g
        work._extra = (mk(), mk())
    Ad, r = work._extra
    g, d, rp = work.g, work.d, work.rp
    # coefficient vectors are opaque to the loop: a device m-vector, or a [w; t] pair for the bound operator Q
    Utr = U.new_coeff() if hasattr(U, "new_coeff") else work.Utr
    Ut = U.adjoint()
    if c is not None:
        U.mul_(x, c)
    else:
        x.fill(0.0)
    r.copy_from(b)
    A.mul_(r, x, 1.0, -1.0)
    g.copy_from(r)
    Ut.mul_(Utr, r)
    U.mul_(g, Utr, -1.0, 1.0)
    r.copy_from(g)
    waxpby(-1.0, g, 0.0, g, d)
    i = 0
    nr = math.inf
    while i < min(maxit, n_global + m):
        i += 1
        A.mul_(Ad, d)
        dAd = dot(d, Ad)
        if dAd <= 0:
            waxpby(1.0 / nrm2(d), d, 0.0, d, x)
            if lam is not None:
                lam.fill(math.nan)
            return i, math.inf
        rg = dot(r, g)
        if rg <= 0:
            break
        alpha = rg / dAd
        axpby(alpha, d, 1.0, x)
        waxpby(1.0, r, alpha, Ad, rp)
        g.copy_from(rp)                      # gp lives in g
        Ut.mul_(Utr, rp)
        U.mul_(g, Utr, -1.0, 1.0)
        beta = dot(rp, g) / rg
        waxpby(beta, d, -1.0, g, d)
        r.copy_from(g)
        nr = nrm2(g)
        if nr < tol:
            break
    r.copy_from(b)
    A.mul_(r, x, -1.0, 1.0)
    if lam is not None:
        Ut.mul_(lam, r)
    return i, nr
