"""projcg! with a SPARSE SYMMETRIC Hessian -- a diagonal plus up to 32 off-diagonal entries per row, described by row indices -- on the one-pass
iteration (lfpsqp_sphess_create, lfpsqp_projcg_sparse, lfpsqp_sphess_mul), and the host layers above it (SparseHessian, SparseOperator,
grid_edges, GraphSeparableLinear).

The distance form (lfpsqp_projcg_stencil) holds 13 distinct distances j - i; the graphs here have 42 (a periodic 3-D grid with corner
neighbours: what grid_laplacian refuses), 1885 and 4050 (triangulated grids in a permuted numbering, 6 neighbours per row) or a row of exactly 32
neighbours.  The reference operator of every check is an independent np.bincount product over the edge list, never the package's builder.
Checked: the builder (widths, duplicates, refusals); the product (plain, stacked, alpha / beta) against a derived rounding bound; counts /
iterates / multipliers against the oracle's projcg! with the same operator as a matrix-free map (materialised and factored bases, dominant and
non-dominant couplings, c != 0, the iteration limit, negative curvature); agreement with lfpsqp_projcg_stencil on the 27-point stencil, with the
callback path, and between two runs; the stacked form under four-way bounds; GraphSeparableLinear through `optimize`; the refusals.

Count comparisons follow the EXIT CONDITION rule of tests/test_projcg_diags.py: the tolerance is `_conditioned_tol`'s (the geometric mean of the
oracle's last two residual norms), and margins of at least 1.1 on both sides are asserted on the oracle alone before the device is looked at."""
import ctypes as C
import math
import sys

import numpy as np
import pytest

import lfpsqp_jl_amd as L
from lfpsqp_jl_amd import _capi
from oracle import lfpsqp_ref as R
from oracle import synth

from .test_capi_retractions import _compare_traces, _note, _sep_host
from .test_projcg_diags import _basis, _conditioned_tol
from .test_projcg_stencil import _edges
from .test_tridiag_bounds import _stacked_problem

KAPPA = 0.9
EPS = 2.0 ** -53


# ---- the test graphs ---------------------------------------------------------------------------------------------------------------------
def _mesh(ny, nx):
    """A triangulated ny x nx grid (edges right, down and down-right) with vertex v renumbered to perm[v]; edges (min, max), sorted."""
    n = ny * nx
    perm = np.argsort(synth.hash_vector(40, n), kind='stable')
    edges = []
    for r in range(ny):
        for c in range(nx):
            v = r * nx + c
            for dr, dc in ((0, 1), (1, 0), (1, 1)):
                if r + dr < ny and c + dc < nx:
                    p, q = int(perm[v]), int(perm[(r + dr) * nx + c + dc])
                    edges.append((min(p, q), max(p, q)))
    return n, sorted(edges)


def _hub(extra=()):
    n = 2300
    edges = [(i, i + 1) for i in range(n - 1)] + [(0, n - 1)] + [(0, 71 * k + 7) for k in range(30)] + list(extra)
    return n, sorted(edges)


_BUILDERS = {"pc567": lambda: (210, _edges((5, 6, 7), True, True)), "pc789": lambda: (504, _edges((7, 8, 9), True, True)),
             "mesh45": lambda: _mesh(45, 50), "mesh70": lambda: _mesh(70, 70), "hub32": _hub,
             "27pt": lambda: (336, _edges((6, 7, 8), False, True)), "mesh266": lambda: _mesh(266, 266)}
# (row width, the edge width the greedy owner rule of include/lfpsqp_hip.h gives: the bound a better rule has to meet, number of distances j - i)
_WIDTHS = {"pc567": (26, 22, 42), "pc789": (26, 22, 42), "mesh45": (6, 5, 1885), "mesh70": (6, 5, 4050), "hub32": (32, 2, None),
           "27pt": (26, 13, 13)}
_GRAPHS = {}


def _graph(name):
    """(n, i, j) of a test graph, i < j in lexicographic order; built once, read-only."""
    if name not in _GRAPHS:
        n, edges = _BUILDERS[name]()
        ei, ej = (np.ascontiguousarray(a) for a in np.array(edges, dtype=np.int64).T)
        assert np.all(ei < ej) and len(set(edges)) == len(edges)
        ei.setflags(write=False)
        ej.setflags(write=False)
        _GRAPHS[name] = (n, ei, ej)
    return _GRAPHS[name]


def _case_operator(name, kind, s=None):
    """(n, i, j, v, a, dominant): A = diag(a) + the entries v_e at (i_e, j_e) and (j_e, i_e).  'lap': v = -w, w_e = 0.9 (0.5 + hash_vector(41)^2)
    on the meshes and 0.9 elsewhere, a = weighted degree + 0.05 + 0.5 hash_vector(3)^2.  'rand': v = s hash_vector(42) of both signs under
    a = 4 hash_vector(3) + 14 -- positive definite, not diagonally dominant."""
    n, ei, ej = _graph(name)
    E = len(ei)
    if kind == "rand":
        return n, ei, ej, s * synth.hash_vector(42, E), 4.0 * synth.hash_vector(3, n) + 14.0, False
    w = KAPPA * (0.5 + synth.hash_vector(41, E) ** 2) if name.startswith("mesh") else np.full(E, KAPPA)
    deg = np.bincount(ei, w, n) + np.bincount(ej, w, n)
    return n, ei, ej, -w, deg + 0.05 + 0.5 * synth.hash_vector(3, n) ** 2, True


class _GraphRef:
    """The reference operator: a np.bincount product over the edge list (stacked: blockdiag(A, diag(ay)))."""

    def __init__(self, n, ei, ej, v, a, ay=None):
        self.n, self.ei, self.ej, self.v, self.a, self.ay = n, ei, ej, v, a, ay

    def _op(self, x):
        n = self.n
        out = self.a * x[:n] + np.bincount(self.ei, self.v * x[self.ej], n) + np.bincount(self.ej, self.v * x[self.ei], n)
        return out if self.ay is None else np.concatenate([out, self.ay * x[n:]])

    def absrow(self, x):
        """|a_i x_i| + sum_j |A_ij x_j| per row: the scale of the product's rounding bound."""
        n = self.n
        return np.abs(self.a * x[:n]) + np.bincount(self.ei, np.abs(self.v * x[self.ej]), n) + np.bincount(self.ej, np.abs(self.v * x[self.ei]), n)

    def mul_(self, dest, x, al=None, be=None):
        t = self._op(x)
        dest[:] = t if al is None else al * t + be * dest
        return dest

    def adjoint(self):
        return self

    def dense(self):
        A = np.diag(self.a)
        np.add.at(A, (self.ei, self.ej), self.v)
        np.add.at(A, (self.ej, self.ei), self.v)
        return A


def _operator(ctx, n, ei, ej, v, a, a0=0.0, ay=None):
    if ay is None:
        dg = ctx.vector(n, a - a0)
    else:
        dg = L.StackedVector(ctx, n).upload2(np.concatenate([a, ay]) - a0)
    return L.SparseOperator(a0, dg, L.SparseHessian(ctx, n, ei, ej, v))


# ---- 1. the builder ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(_WIDTHS))
def test_builder_and_info(dev_ctx, name):
    ctx = dev_ctx
    n, ei, ej = _graph(name)
    kr, ke_max, ndist = _WIDTHS[name]
    if ndist is not None:
        assert len(set((ej - ei).tolist())) == ndist
    assert np.bincount(np.concatenate([ei, ej]), minlength=n).max() == kr
    order = np.argsort(synth.hash_vector(43, len(ei)), kind='stable')            # the triplets in any order, some of them mirrored
    flip = synth.hash_vector(44, len(ei)) > 0
    gi, gj = np.where(flip, ej, ei)[order], np.where(flip, ei, ej)[order]
    S = L.SparseHessian(ctx, n, gi, gj, -KAPPA)
    print(f"[sphess] {name}: n={S.n} edges={S.nedges} row width {S.row_width} edge width {S.edge_width}")
    assert (S.n, S.nedges, S.row_width) == (n, len(ei), kr)
    assert S.edge_width <= ke_max and S.edge_width * n >= S.nedges
    S.close()
    S.close()                                                        # (closing twice is harmless)


def test_builder_merges_duplicates_and_refuses(dev_ctx):
    ctx = dev_ctx
    n = 40
    # (0, 5) three times, once mirrored; (3, 4) twice with the sum zero: it keeps its slot
    i = np.array([0, 0, 3, 3, 10, 38, 5, 0, 4])
    j = np.array([1, 5, 4, 8, 39, 39, 0, 5, 3])
    w = np.array([1.0, 2.0, -3.0, 0.5, 4.0, 7.0, 0.25, 0.125, 3.0])
    S = L.SparseHessian(ctx, n, i, j, w)
    assert (S.n, S.nedges, S.row_width, S.edge_width) == (n, 6, 2, 1)
    A = np.zeros((n, n))
    for a, b, ww in zip(i, j, w):
        A[a, b] += ww
        A[b, a] += ww
    assert A[3, 4] == 0.0 and A[0, 5] == 2.375
    vh = synth.hash_vector(7, n)
    out = ctx.vector(n)
    L.SparseOperator(0.0, None, S).mul_(out, ctx.vector(n, vh))
    assert np.abs(out.download() - A @ vh).max() <= 4 * EPS * np.abs(A).sum(axis=1).max()
    S0 = L.SparseHessian(ctx, 5, [], [], 1.0)                      # no edges at all
    assert (S0.n, S0.nedges, S0.row_width, S0.edge_width) == (5, 0, 0, 0)

    def create(n_, ii, jj, vv):
        ii, jj, vv = (np.ascontiguousarray(x, dtype=t) for x, t in ((ii, np.int64), (jj, np.int64), (vv, np.float64)))
        h = C.c_void_p()
        rc = ctx.L.lfpsqp_sphess_create(ctx.h, n_, len(ii), ii.ctypes.data, jj.ctypes.data, vv.ctypes.data, C.byref(h))
        if rc == 0:
            ctx.L.lfpsqp_sphess_free(ctx.h, h)
        return rc
    assert create(10, [1, 2], [2, 3], [1.0, 1.0]) == 0
    assert create(10, [1, 2], [2, 2], [1.0, 1.0]) == -1              # i == j: the diagonal is dg's job
    assert create(10, [1, 10], [2, 3], [1.0, 1.0]) == -1             # an index outside [0, n)
    assert create(10, [1, 2], [2, -1], [1.0, 1.0]) == -1
    assert create(10, [1, 2], [2, 3], [1.0, np.nan]) == -1           # a non-finite value
    assert create(10, [1, 2], [2, 3], [np.inf, 1.0]) == -1
    assert create(2 ** 31, [], [], []) == -5                         # indices are stored as int32
    assert create(2 ** 31 - 1, [1, 2], [2, 2], [1.0, 1.0]) == -1     # (the widest n is looked at: its entries are checked)
    n32, e32 = _hub()
    ei, ej = np.array(e32).T
    S32 = L.SparseHessian(ctx, n32, ei, ej, 1.0)
    assert S32.row_width == 32
    n33, e33 = _hub(extra=[(0, 3)])
    ei, ej = np.array(e33).T
    assert create(n33, ei, ej, np.ones(len(ei))) == -5               # 33 distinct neighbours
    with pytest.raises(L.LfpsqpError):
        L.SparseHessian(ctx, n33, ei, ej, 1.0)
    ei, ej = np.array(e32 + [(7, 0), (0, 7), (1, 0)]).T               # 32 after merging: accepted
    assert create(n32, ei, ej, np.ones(len(ei))) == 0


# ---- 2. the product ----------------------------------------------------------------------------------------------------------------------
def _product_bound(ref, x, kr):
    """2 (Kr + 2) 2^-53 (|a_i x_i| + sum_j |A_ij x_j|) per row: Kr + 2 roundings in the device's fma chain (a0 + dg_i, the first product, one per
    slot) plus as many in the numpy reference."""
    return 2.0 * (kr + 2) * EPS * ref.absrow(x)


@pytest.mark.parametrize("name", list(_WIDTHS))
def test_sparse_product(dev_ctx, name):
    ctx = dev_ctx
    kr = _WIDTHS[name][0]
    kind, s = ("rand", 3.5) if name.startswith("mesh") else ("lap", None)
    n, ei, ej, v, a, _ = _case_operator(name, kind, s)
    ref = _GraphRef(n, ei, ej, v, a)
    vh = synth.hash_vector(7, n)
    A = _operator(ctx, n, ei, ej, v, a, a0=0.25)
    assert A.S.row_width == kr
    out = ctx.vector(n)
    A.mul_(out, ctx.vector(n, vh))
    want = ref._op(vh)
    bound = _product_bound(ref, vh, kr)
    err = np.abs(out.download() - want)
    print(f"[sparse product] {name}: max error / bound {np.max(err / bound):.2f}")
    assert np.all(err <= bound)
    out.upload(np.ones(n))
    A.mul_(out, ctx.vector(n, vh), 2.0, -1.0)                       # mul!(dest, A, v, alpha, beta)
    # (twice the product's error, plus the two roundings of 2 t - 1)
    assert np.all(np.abs(out.download() - (2.0 * want - 1.0)) <= 2.0 * bound + 2 * EPS * (np.abs(2.0 * want) + 1.0))
    # stacked pair: the couplings on the x half, the y half diagonal, the gap left at zero
    ay = synth.hash_vector(16, n)
    vs = synth.hash_vector(8, 2 * n)
    As = _operator(ctx, n, ei, ej, v, a, a0=0.25, ay=ay)
    outs = L.StackedVector(ctx, n)
    As.mul_(outs, L.StackedVector(ctx, n).upload2(vs))
    refs = _GraphRef(n, ei, ej, v, a, ay)
    errs = np.abs(outs.download2() - refs._op(vs))
    assert np.all(errs[:n] <= _product_bound(refs, vs, kr))
    assert np.all(errs[n:] <= 4 * EPS * (np.abs(ay) + 0.5) * np.abs(vs[n:]))       # (ay - a0, a0 + dg, the product; a0 = 0.25)
    assert not np.any(outs.download(outs.hs - n, n))


# ---- 3. solves on one pass ---------------------------------------------------------------------------------------------------------------
_ORACLE = {}
_LMIN = {}


def _oracle_solve(key, Aref, Uh, bh, c0, m):
    """`_conditioned_tol`'s (tol, count, margins) and the oracle's solve at that tolerance; once per case, shared by the emulator and GPU runs."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    tol, i_base, up, down = _conditioned_tol(Aref, Uh, bh, c0, m)
    x0, l0 = np.zeros(len(bh)), np.zeros(m)
    i0, nr0 = R.projcg_(x0, l0, Aref, Uh, bh, c0.copy(), tol=tol)
    x0.setflags(write=False)
    l0.setflags(write=False)
    res = (tol, i_base, up, down, x0, l0, i0, nr0)
    if key is not None:
        _ORACLE[key] = res
    return res


# (graph, operator, s, m, factored, the oracle's count at tol = 1e-10 for c = 0 with U = qr(hash_matrix(1, n, m)), b = hash_vector(4, n))
_CASES = [("pc567", "lap", None, 6, False, 25), ("pc789", "lap", None, 33, False, 31), ("mesh45", "lap", None, 33, False, 80),
          ("mesh70", "lap", None, 130, False, 81), ("hub32", "lap", None, 6, False, 82),
          ("mesh45", "rand", 3.5, 33, False, 39), ("mesh70", "rand", 3.5, 130, False, 39), ("pc567", "rand", 1.2, 6, False, 21),
          ("mesh45", "lap", None, 33, True, None), ("pc567", "lap", None, 6, True, None), ("mesh70", "rand", 3.5, 130, True, None)]


# The one graph on which the ORACLE's count moves with the BLAS kernels numpy runs on (the docstring of the test has the figures).  Its solves
# run with b = hash_vector(4, n) wherever the oracle's margins with it reach 1.1, and with the next seed that reaches them only where they do not.
_BLAS_SENSITIVE = {"hub32"}


@pytest.mark.parametrize("name,kind,s,m,factored,count", _CASES)
def test_projcg_with_a_sparse_hessian_on_one_pass(dev_ctx, name, kind, s, m, factored, count):
    """The 'rand' data (dense check with numpy, not the code under test): 327, 675 and 150 rows with a negative Gram weight c_i, lambda_min =
    1.86, 2.41 and 6.08 on mesh45, mesh70 and pc567.
    hub32 (a ring of 2300 with 30 spokes; 82 to 84 iterations): the oracle's OWN count moves with the kernels OpenBLAS dispatches to for numpy's
    qr and products (OPENBLAS_CORETYPE forces a family).  Iterations / smaller margin of the oracle with b = hash_vector(4, n), c = 0 and c given:
    SkylakeX (a CPU with AVX-512) 82 / 1.20 and 83 / 1.08; Haswell 83 / 1.05 and 82 / 1.20; Sandybridge 82 / 1.20 and 82 / 1.11; Nehalem
    83 / 1.73 and 82 / 1.15.  With hash_vector(5, n): 82 / 1.20 and 82 / 1.20 under SkylakeX and Haswell.  Where the oracle misses the margin of
    1.1 this file asks of it before it looks at the device, a comparison of counts would test the last bits of the oracle's norms; such a solve
    takes the next seed of b whose margins reach 1.1 and says so in its output -- decided on the oracle alone.  Where seed 4 meets the margin the
    solve runs as named, and for c = 0 its count is held against the 82 of the case list (which the Nehalem kernels do not give)."""
    ctx = dev_ctx
    n, ei, ej, v, a, dominant = _case_operator(name, kind, s)
    Aref = _GraphRef(n, ei, ej, v, a)
    if not dominant:
        cw = a - np.bincount(ei, np.abs(v), n) - np.bincount(ej, np.abs(v), n)
        if (name, s) not in _LMIN:
            _LMIN[(name, s)] = float(np.linalg.eigvalsh(Aref.dense())[0])
        print(f"[sparse] {name} {np.count_nonzero(cw < 0)} negative Gram weights, lambda_min = {_LMIN[(name, s)]:.3f}")
        assert np.any(cw < 0)                                        # some Gram weight c_i is negative: the extra pass runs
        assert _LMIN[(name, s)] > 0.05
    U, Uh = _basis(ctx, n, m, factored)
    A = _operator(ctx, n, ei, ej, v, a)
    bh = synth.hash_vector(4, n)
    b = ctx.vector(n, bh)
    work = L.ProjCGWork(ctx, n, m)
    for ch in (None, np.linspace(-1, 1, m)):
        c0 = np.zeros(m) if ch is None else ch
        bh = synth.hash_vector(4, n)
        b = ctx.vector(n, bh)
        key = None if factored else (name, kind, s, m, ch is None)   # (the factored basis comes from the device's own ksvd_)
        tol, i_base, up, down, x0, l0, i0, nr0 = _oracle_solve(key, Aref, Uh, bh, c0, m)
        seed = 4
        while name in _BLAS_SENSITIVE and min(up, down) < 1.1 and seed < 8:
            seed += 1
            print(f"[sparse] {name}: the oracle's margins are {up:.2f} / {down:.2f} under this BLAS: b = hash_vector({seed}, n)")
            bh = synth.hash_vector(seed, n)
            b = ctx.vector(n, bh)
            tol, i_base, up, down, x0, l0, i0, nr0 = _oracle_solve(key + (seed,), Aref, Uh, bh, c0, m)
        print(f"[sparse] {name} {kind} m={m} factored={factored} c={'0' if ch is None else 'given'}: oracle {i_base} iterations at 1e-10, "
              f"tol {tol:.3e}, margins {up:.2f} / {down:.2f}")
        if ch is None and count is not None and seed == 4:
            assert i_base == count
        assert up >= 1.1 and down >= 1.1
        assert i0 == i_base
        x, lam = ctx.vector(n), ctx.vector(m)
        i1, nr1 = L.projcg_(x, lam, A, U, b, None if ch is None else ctx.vector(m, ch), tol=tol, work=work)
        dx = np.linalg.norm(x.download() - x0) / np.linalg.norm(x0)
        dl = np.abs(lam.download() - l0).max()
        print(f"[sparse]   iterations {i1} (oracle {i0}), nr {nr1:.6e} ({nr0:.6e}), x {dx:.1e}, lambda {dl:.1e}")
        assert i1 == i0 and i1 > 3 and nr1 == pytest.approx(nr0, rel=1e-5)
        assert dx <= 1e-10
        assert dl <= 1e-10
    # the iteration limit (src/projcg.jl:71)
    bh = synth.hash_vector(4, n)
    b = ctx.vector(n, bh)
    x0, l0 = np.zeros(n), np.zeros(m)
    i0, nr0 = R.projcg_(x0, l0, Aref, Uh, bh, np.zeros(m), tol=1e-30, maxit=5)
    x, lam = ctx.vector(n), ctx.vector(m)
    i1, nr1 = L.projcg_(x, lam, A, U, b, None, tol=1e-30, maxit=5, work=work)
    assert (i1, i0) == (5, 5) and nr1 == pytest.approx(nr0, rel=1e-9)
    assert np.linalg.norm(x.download() - x0) <= 1e-12 * np.linalg.norm(x0)
    # negative curvature (src/projcg.jl:77-82)
    x0, l0 = np.zeros(n), np.zeros(m)
    i0, nr0 = R.projcg_(x0, l0, _GraphRef(n, ei, ej, v, -a), Uh, bh, np.zeros(m), tol=1e-10)
    x, lam = ctx.vector(n), ctx.vector(m)
    i1, nr1 = L.projcg_(x, lam, _operator(ctx, n, ei, ej, v, -a), U, b, None, tol=1e-10, work=work)
    assert (i1, nr1) == (i0, nr0) and math.isinf(nr1)
    assert np.linalg.norm(x.download() - x0) <= 1e-10 and np.all(np.isnan(lam.download()))


# ---- 4. agreement with what exists -------------------------------------------------------------------------------------------------------
def test_sparse_entry_agrees_with_the_stencil_entry_on_the_27_point_stencil(dev_ctx):
    ctx = dev_ctx
    m = 6
    n, ei, ej, v, a, _ = _case_operator("27pt", "lap")
    Aref = _GraphRef(n, ei, ej, v, a)
    A = _operator(ctx, n, ei, ej, v, a)
    diag, off, dists = L.graph_diagonals(n, ei, ej, KAPPA)
    assert len(dists) == 13
    Ast = L.DiagonalsOperator(0.0, ctx.vector(n, a), ctx.matrix(n, 13, off), dists)
    U, Uh = _basis(ctx, n, m, False)
    bh = synth.hash_vector(4, n)
    b = ctx.vector(n, bh)
    for ch in (None, np.linspace(-1, 1, m)):
        tol, i_base, up, down = _conditioned_tol(Aref, Uh, bh, np.zeros(m) if ch is None else ch, m)
        print(f"[sparse vs stencil] c={'0' if ch is None else 'given'}: oracle {i_base} iterations, margins {up:.2f} / {down:.2f}")
        assert up >= 1.1 and down >= 1.1
        res = []
        for op in (A, Ast):
            x, lam = ctx.vector(n), ctx.vector(m)
            it, nr = L.projcg_(x, lam, op, U, b, None if ch is None else ctx.vector(m, ch), tol=tol, work=L.ProjCGWork(ctx, n, m))
            res.append((it, x.download(), lam.download()))
        assert res[0][0] == res[1][0] == i_base
        assert np.linalg.norm(res[0][1] - res[1][1]) <= 1e-10 * np.linalg.norm(res[1][1])
        assert np.abs(res[0][2] - res[1][2]).max() <= 1e-10


def test_callback_path_agrees_and_runs_repeat_bit_for_bit(dev_ctx):
    ctx = dev_ctx
    m = 33
    n, ei, ej, v, a, _ = _case_operator("mesh45", "lap")
    A = _operator(ctx, n, ei, ej, v, a)
    U, Uh = _basis(ctx, n, m, False)
    bh = synth.hash_vector(4, n)
    b = ctx.vector(n, bh)
    tol, i_base, up, down, *_ = _oracle_solve(("mesh45", "lap", None, m, True), _GraphRef(n, ei, ej, v, a), Uh, bh, np.zeros(m), m)
    assert up >= 1.1 and down >= 1.1
    res = []
    for fused in (True, True, False):
        A.fused = fused
        x, lam = ctx.vector(n), ctx.vector(m)
        it, nr = L.projcg_(x, lam, A, U, b, None, tol=tol, work=L.ProjCGWork(ctx, n, m))
        res.append((it, nr, x.download(), lam.download()))
    A.fused = True
    assert res[0][0] == res[2][0] == i_base
    assert np.linalg.norm(res[0][2] - res[2][2]) <= 1e-10 * np.linalg.norm(res[0][2])
    assert np.abs(res[0][3] - res[2][3]).max() <= 1e-10
    # two solves of the same problem: identical bits
    assert res[0][:2] == res[1][:2] and np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


# ---- 5. bounds ---------------------------------------------------------------------------------------------------------------------------
def _solve_stacked_c(ctx, A, P, b, n, m, tol, maxit=None):
    """lfpsqp_projcg_sparse itself over a stacked basis (no fall-back): rc, iterations, nr, x, lambda."""
    x, lam = L.StackedVector(ctx, n), ctx.vector(n + m)
    work = L.ProjCGWork(ctx, 0, m, stacked_N=n)
    Av = L.StackedVector(ctx, n)
    it, nr = _capi.c_i64(), C.c_double()
    u_c, w_c = P._c(), work._c()
    rc = ctx.L.lfpsqp_projcg_sparse(ctx.h, x.h, lam.h, A.a0, A.dg.h, A.S.h, Av.h, C.byref(u_c), b.h, None, float(tol),
                                    int(2 * n + m if maxit is None else maxit), 2 * n, 1, C.byref(w_c), C.byref(it), C.byref(nr))
    return rc, it.value, nr.value, x, lam


# (graph, m, factored, the seed of b: the first of 4, 5, ... whose oracle margins reach 1.1)
@pytest.mark.parametrize("name,m,factored,seed", [("pc567", 16, False, 4), ("mesh45", 33, False, 4), ("pc567", 16, True, 4)])
def test_stacked_sparse_solver_follows_the_oracle(dev_ctx, name, m, factored, seed):
    """Four-way bounds: lfpsqp_projcg_sparse over a stacked basis against the oracle's projcg! with the augmented map blockdiag(A, diag(ay))."""
    ctx = dev_ctx
    n, ei, ej, v, ax, _ = _case_operator(name, "lap")
    P, P0, _, rank = _stacked_problem(ctx, n, m, factored)
    assert rank == m
    ay = 0.5 + synth.hash_vector(16, n) ** 2
    A = _operator(ctx, n, ei, ej, v, ax, ay=ay)
    Aref = _GraphRef(n, ei, ej, v, ax, ay)
    bh = synth.hash_vector(seed, 2 * n)
    tmp = np.zeros(n + m)
    R.mul_(tmp, R.adj(P0), bh)
    R.mul_(bh, P0, tmp, -1.0, 1.0)                                      # a right-hand side in the tangent space, like optimize's d
    b = L.StackedVector(ctx, n).upload2(bh)
    tol_c, i_base, up, down = _conditioned_tol(Aref, P0, bh, np.zeros(n + m), n + m)
    print(f"[stacked sparse] {name} m={m} factored={factored} seed={seed}: oracle {i_base} iterations at 1e-10, tol {tol_c:.3e}, margins {up:.2f} / {down:.2f}")
    assert up >= 1.1 and down >= 1.1
    for tol, maxit in ((tol_c, None), (1e-300, 5)):
        x0, l0 = np.zeros(2 * n), np.zeros(n + m)
        i0, nr0 = R.projcg_(x0, l0, Aref, P0, bh, np.zeros(n + m), tol=tol, maxit=maxit)
        rc, i1, nr1, x, lam = _solve_stacked_c(ctx, A, P, b, n, m, tol, maxit)
        assert rc == 0
        xd, ld = x.download2(), lam.download()
        dx_ = np.linalg.norm(xd - x0) / np.linalg.norm(x0)
        dl_ = np.abs(ld - l0).max() / np.abs(l0).max()
        print(f"[stacked sparse]   maxit={maxit}: iterations {i1} (oracle {i0}), nr {nr1:.6e} ({nr0:.6e}), x {dx_:.1e}, lambda {dl_:.1e}")
        assert i1 == i0 and (maxit is not None or (i1 == i_base and i1 > 3))
        assert dx_ <= 1e-10 and dl_ <= 1e-9
    # negative curvature
    x0, l0 = np.zeros(2 * n), np.zeros(n + m)
    i0, nr0 = R.projcg_(x0, l0, _GraphRef(n, ei, ej, v, -ax, ay), P0, bh, np.zeros(n + m), tol=1e-10)
    rc, i1, nr1, x, lam = _solve_stacked_c(ctx, _operator(ctx, n, ei, ej, v, -ax, ay=ay), P, b, n, m, 1e-10)
    assert rc == 0 and (i1, nr1) == (i0, nr0) and math.isinf(nr1)
    assert np.all(np.isnan(lam.download()))


# ---- 6. optimize -------------------------------------------------------------------------------------------------------------------------
def test_graph_objective_follows_the_oracle(dev_ctx):
    """GraphSeparableLinear on the 26-neighbour periodic grid with ball and box through `optimize`: every truncated-Newton solve runs a
    SparseOperator from the tangent step's state on lfpsqp_projcg_sparse, and the trajectory is the oracle's with hess_lag_vec! a matrix-free
    map over the edge list.  The oracle is run a second time from one ulp away, as in tests/test_projcg_stencil.py."""
    ctx = dev_ctx
    n, ei, ej = _graph("pc567")
    m, maxiter, kind = 4, 8, 1
    lap = _GraphRef(n, ei, ej, np.full(len(ei), -KAPPA), np.bincount(np.concatenate([ei, ej]), minlength=n) * KAPPA)
    pen = lap._op
    a = 0.5 + synth.hash_vector(21, n) ** 2
    c = 1.3 * synth.hash_vector(22, n)
    phi, d1, d2 = _sep_host(kind, a, c)
    P0 = synth.BallBoxProblem(n, m)
    x0 = 0.9 * synth.hash_vector(2, n) + 0.05
    f = lambda x: float(np.sum(phi(x[:n])) + 0.5 * KAPPA * np.sum((x[ei] - x[ej]) ** 2))

    def grad_(g, x):
        g[:n] = d1(x[:n]) + pen(x[:n])

    def hlv_(dest, src, x, lam):
        dest[:] = (d2(x) + 2.0 * lam[m]) * src + pen(src)
    par = dict(do_project_retract=False, maxiter=maxiter, tn_kappa=1e-6)

    def oracle(xs, trace):
        p = R.LFPSQPParams(disp=R.DisplayOption.off, **par)
        dv0 = P0.derivatives()
        return R.optimize(f, P0.c_, P0.d_, xs, P0.xl, P0.xu, m, 1, p,
                          derivatives=R.Derivatives(grad_=grad_, hess_lag_vec_=hlv_, jac_c_=dv0.jac_c_, jac_d_=dv0.jac_d_), trace=trace)
    tr0, tr1, tr = [], [], []
    xr, objr, lamr, tir = oracle(x0, tr0)
    oracle(np.nextafter(x0, np.inf), tr1)
    sens = [np.linalg.norm(p['x'] - q['x']) / np.linalg.norm(q['x']) for p, q in zip(tr1, tr0)] + [np.inf] * (len(tr0) - len(tr1))
    P = L.GraphSeparableLinear(ctx, n, m, ctx.matrix(n + 1, m + 1).hash_fill(1, 0, n, 1.0, n, m), P0.eq.b, kind, a, c, edges=(ei, ej, 1.0),
                               kappa=KAPPA, R2=P0.R2, xl=P0.xl, xu=P0.xu)
    S = P.sparse_hessian
    assert (S.n, S.nedges, S.row_width) == (n + 1, len(ei), 26)    # (the slack row has no couplings)
    OPT = sys.modules["lfpsqp_jl_amd.optimize"]
    seen, rcs, orig = [], [], OPT.projcg_
    c_entry = ctx.L.lfpsqp_projcg_sparse

    def spy(*args, **kw):
        seen.append((type(args[2]).__name__, bool(kw.get("start_given"))))
        return orig(*args, **kw)

    def c_spy(*args):
        rc = c_entry(*args)
        rcs.append(rc)
        return rc
    OPT.projcg_ = spy
    setattr(ctx.L, "lfpsqp_projcg_sparse", c_spy)
    try:
        x, obj, lam, ti = P.optimize(x0, L.LFPSQPParams(disp=L.DisplayOption.off, **par), trace=tr)
    finally:
        OPT.projcg_ = orig
        setattr(ctx.L, "lfpsqp_projcg_sparse", c_entry)
    assert seen and all(s == ("SparseOperator", True) for s in seen)
    assert len(rcs) == len(seen) and all(rc == 0 for rc in rcs)
    assert ti.iter == tir.iter and ti.condition.name == tir.condition.name
    print("[graph objective pc567] Newton-system iterations", [t.get('tn_iter') for t in tr0])
    assert any((t.get('tn_iter') or 0) >= 2 for t in tr0)            # (from the second iteration on the one-pass kernel itself runs)
    rtol = max(1e-10, 10.0 * max(sens))
    _note(f"graph objective pc567: the oracle's one-ulp sensitivity {max(sens):.1e}")
    assert max(sens) <= 1e-12                                        # (the comparison below is at 1e-10, not at the oracle's own spread)
    assert _compare_traces(tr, tr0, rtol=rtol) is None
    assert abs(obj[-1] - objr[-1]) <= 1e-11 * abs(objr[-1])
    assert np.linalg.norm(x - xr) <= 1e-10 * np.linalg.norm(xr)


def test_grid_edges_is_the_public_edge_list():
    for shape, per, corners in (((5, 6, 7), True, True), ((6, 7, 8), False, True), ((4, 5), (True, False), False)):
        gi, gj = L.grid_edges(shape, periodic=per, corners=corners)
        assert sorted(zip(gi.tolist(), gj.tolist())) == _edges(shape, per, corners)
    gi, gj = L.grid_edges((5, 6, 7), True, True)
    assert len(gi) == 2730 and len(set((gj - gi).tolist())) == 42
    with pytest.raises(ValueError, match=r"\b\d\d distinct"):         # ... which the distance form still refuses
        L.grid_laplacian((5, 6, 7), 1.0, periodic=True, corners=True)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_sparse_entries_refuse_what_has_no_one_pass_form(dev_ctx):
    ctx = dev_ctx
    m = 8
    n, ei, ej, v, a, _ = _case_operator("pc567", "lap")
    A = _operator(ctx, n, ei, ej, v, a)
    dg = A.dg
    b = ctx.vector(n, synth.hash_vector(4, n))
    Ssmall = L.SparseHessian(ctx, n - 1, [0], [1], 1.0)
    for view in (False, True):
        Uh, _ = np.linalg.qr(synth.hash_matrix(1, n, m))
        Zd = ctx.matrix(n, m, np.asfortranarray(Uh))
        U = L.DeviceBasis(Zd.view(ctx.vector(n, np.ones(n))) if view else Zd)
        x, lam, Av = ctx.vector(n), ctx.vector(m), ctx.vector(n)
        work = L.ProjCGWork(ctx, n, m)
        it, nr = _capi.c_i64(), C.c_double()
        u_c, w_c = U._c(), work._c()

        def solve(flags=1, S=A.S.h):
            return ctx.L.lfpsqp_projcg_sparse(ctx.h, x.h, lam.h, 0.0, dg.h, S, Av.h, C.byref(u_c), b.h, None, 1e-10, 100, n, flags,
                                              C.byref(w_c), C.byref(it), C.byref(nr))
        if view:
            assert solve() == -5                                    # LFPSQP_ERR_UNSUPPORTED: a matrix view as basis
            continue
        assert solve(flags=1 | L.projcg.RESUME) == -1
        assert solve(flags=1 | L.projcg.START_PROJECTED) == -1
        assert solve(S=None) == -1
        assert solve(S=Ssmall.h) == -1                              # S of the wrong row count
        assert ctx.L.lfpsqp_sphess_mul(ctx.h, 0.0, dg.h, Ssmall.h, b.h, Av.h) == -1
        assert ctx.L.lfpsqp_sphess_mul(ctx.h, 0.0, dg.h, None, b.h, Av.h) == -1
        assert solve() == 0 and it.value > 3
        assert ctx.L.lfpsqp_sphess_mul(ctx.h, 0.0, dg.h, A.S.h, b.h, Av.h) == 0
    # too few columns for the one-pass kernels
    U3 = L.DeviceBasis(ctx.matrix(n, 3, np.asfortranarray(np.linalg.qr(synth.hash_matrix(1, n, 3))[0])))
    x, lam, Av = ctx.vector(n), ctx.vector(3), ctx.vector(n)
    work = L.ProjCGWork(ctx, n, 3)
    it, nr = _capi.c_i64(), C.c_double()
    u_c, w_c = U3._c(), work._c()
    assert ctx.L.lfpsqp_projcg_sparse(ctx.h, x.h, lam.h, 0.0, dg.h, A.S.h, Av.h, C.byref(u_c), b.h, None, 1e-10, 100, n, 1, C.byref(w_c),
                                      C.byref(it), C.byref(nr)) == -5
    # c != 0 with a stacked basis
    P, _, _, _ = _stacked_problem(ctx, n, m, False)
    As = _operator(ctx, n, ei, ej, v, a, ay=np.ones(n))
    xs, lams, Avs = L.StackedVector(ctx, n), ctx.vector(n + m), L.StackedVector(ctx, n)
    works = L.ProjCGWork(ctx, 0, m, stacked_N=n)
    u_c, w_c = P._c(), works._c()
    bs = L.StackedVector(ctx, n).upload2(synth.hash_vector(4, 2 * n))
    rc = ctx.L.lfpsqp_projcg_sparse(ctx.h, xs.h, lams.h, 0.0, As.dg.h, As.S.h, Avs.h, C.byref(u_c), bs.h, ctx.vector(m, np.ones(m)).h, 1e-10, 100,
                                    2 * n, 1, C.byref(w_c), C.byref(it), C.byref(nr))
    assert rc == -5


def test_sparse_entries_refuse_row_shards_and_foreign_handles(emu_lib):
    """A communicator (the row-shard case): the one-pass solve and the product answer LFPSQP_ERR_UNSUPPORTED; projcg_ raises.  A handle built on
    another context is refused by SparseOperator."""
    ctx = L.Context(0, emu_lib)
    ctx2 = L.Context(0, emu_lib)
    try:
        m = 8
        n, ei, ej, v, a, _ = _case_operator("pc567", "lap")
        S2 = L.SparseHessian(ctx2, n, ei, ej, v)
        with pytest.raises(ValueError):
            L.SparseOperator(0.0, ctx.vector(n, a), S2)
        with pytest.raises(ValueError):
            L.SparseOperator(0.0, None, S2).mul_(ctx.vector(n), ctx.vector(n))
        S2.close()
        ctx.comm_init_callback(0, 1, lambda ptr, count, op, stream: 0)
        A = _operator(ctx, n, ei, ej, v, a)
        Uh, _ = np.linalg.qr(synth.hash_matrix(1, n, m))
        U = L.DeviceBasis(ctx.matrix(n, m, np.asfortranarray(Uh)))
        b, x, lam, Av = ctx.vector(n, synth.hash_vector(4, n)), ctx.vector(n), ctx.vector(m), ctx.vector(n)
        work = L.ProjCGWork(ctx, n, m)
        it, nr = _capi.c_i64(), C.c_double()
        u_c, w_c = U._c(), work._c()
        rc = ctx.L.lfpsqp_projcg_sparse(ctx.h, x.h, lam.h, 0.0, A.dg.h, A.S.h, Av.h, C.byref(u_c), b.h, None, 1e-10, 100, n, 1, C.byref(w_c),
                                        C.byref(it), C.byref(nr))
        assert rc == -5
        assert ctx.L.lfpsqp_sphess_mul(ctx.h, 0.0, A.dg.h, A.S.h, b.h, Av.h) == -5
        with pytest.raises(L.LfpsqpError):
            L.projcg_(x, lam, A, U, b, None, tol=1e-10, work=work)
    finally:
        ctx2.close()
        ctx.close()


# ---- 8. a size at which a workgroup of the vector launches takes several rounds --------------------------------------------------------------
@pytest.mark.gpu
def test_sparse_at_a_size_of_several_rounds(gpu_lib):
    """A 266 x 266 permuted mesh, n = 70756, m = 16: the product against the bincount reference, a solve capped at 30 iterations against the
    oracle."""
    ctx = L.Context(0, gpu_lib)
    try:
        m = 16
        n, ei, ej, v, a, _ = _case_operator("mesh266", "lap")
        assert n == 70756
        A = _operator(ctx, n, ei, ej, v, a)
        assert A.S.row_width == 6
        ref = _GraphRef(n, ei, ej, v, a)
        vh = synth.hash_vector(7, n)
        out = ctx.vector(n)
        A.mul_(out, ctx.vector(n, vh))
        assert np.all(np.abs(out.download() - ref._op(vh)) <= _product_bound(ref, vh, 6))
        U, Uh = _basis(ctx, n, m, False)
        bh = synth.hash_vector(4, n)
        x0, l0 = np.zeros(n), np.zeros(m)
        i0, nr0 = R.projcg_(x0, l0, ref, Uh, bh, np.zeros(m), tol=1e-300, maxit=30)
        x, lam = ctx.vector(n), ctx.vector(m)
        i1, nr1 = L.projcg_(x, lam, A, U, ctx.vector(n, bh), None, tol=1e-300, maxit=30, work=L.ProjCGWork(ctx, n, m))
        dx = np.linalg.norm(x.download() - x0) / np.linalg.norm(x0)
        dl = np.abs(lam.download() - l0).max()
        print(f"[sparse 70756] iterations {i1} (oracle {i0}), nr {nr1:.6e} ({nr0:.6e}), x {dx:.1e}, lambda {dl:.1e}")
        assert (i1, i0) == (30, 30) and nr1 == pytest.approx(nr0, rel=1e-5)
        assert dx <= 1e-10 and dl <= 1e-10
    finally:
        ctx.close()
