"""projcg! with a WIDE grid-stencil Hessian -- a diagonal plus up to THIRTEEN off-diagonals at arbitrary distances -- on the one-pass iteration
(lfpsqp_projcg_stencil, lfpsqp_stencil_mul), and the host builders that produce such operators from a grid description.

The 27-point stencil of a 3-D field has 13 off-diagonals; a periodic axis adds no new operator form (a wrap-around edge between rows i < j is
one more entry at distance j - i) but more distances: 4 for the periodic 5-point stencil, 6 for the periodic 7-point one, 10 for the periodic
2-D stencil with corner neighbours.  Checked here: the builders (`grid_laplacian` with `periodic` / `corners`, `graph_diagonals`) against an
independent construction; the product on 5, 8 and 13 distances below and beyond a 2048-row tile (plain, stacked, ignored entries poisoned);
counts / iterates / multipliers against the oracle's projcg! with the same operator as a matrix-free map (materialised and factored bases,
dominant and non-dominant couplings, c != 0, the iteration limit, negative curvature); bit-identity with lfpsqp_projcg_diags / lfpsqp_diags_mul
for K <= 4; the callback path; the stacked form under four-way bounds; GridSeparableLinear through `optimize`; the refusals.

Count comparisons follow the EXIT CONDITION rule of tests/test_projcg_diags.py: the tolerance is `_conditioned_tol`'s (the geometric mean of the
oracle's last two residual norms), and margins of at least 1.1 on both sides are asserted on the oracle alone before the device is looked at.
The oracle's counts at tol = 1e-10 (U = qr(hash_matrix(1, n, m)), b = hash_vector(4, n), a = deg + 0.05 + 0.5 hash_vector(3, n)^2, kappa = 0.9,
c = 0) are asserted per case."""
import ctypes as C
import itertools
import math
import sys

import numpy as np
import pytest

import lfpsqp_jl_amd as L
from lfpsqp_jl_amd import _capi
from oracle import lfpsqp_ref as R
from oracle import synth

from .test_capi_retractions import _compare_traces, _note, _sep_host
from .test_projcg_diags import _apply, _basis, _conditioned_tol, _dense, _DiagsRef, _off_matrix, _operator
from .test_tridiag_bounds import _stacked_problem

KAPPA = 0.9
_STENCILS = {"27": dict(corners=True), "per": dict(periodic=True), "percorn": dict(periodic=True, corners=True)}


def _edges(shape, periodic, corners):
    """The edge set of the grid graph, point by point: a loop over the coordinate offsets with np.ravel_multi_index (independent of the
    package's vectorised builder).  A set, so an edge named twice counts once."""
    d = len(shape)
    per = (periodic,) * d if isinstance(periodic, bool) else tuple(periodic)
    if corners:
        offsets = [o for o in itertools.product((-1, 0, 1), repeat=d) if any(o)]
    else:
        offsets = [tuple(sg * int(ax == k) for k in range(d)) for ax in range(d) for sg in (-1, 1)]
    edges = set()
    for p in itertools.product(*(range(s) for s in shape)):
        i = int(np.ravel_multi_index(p, shape))
        for o in offsets:
            q = []
            for ax in range(d):
                c = p[ax] + o[ax]
                if per[ax]:
                    c %= shape[ax]
                elif not 0 <= c < shape[ax]:
                    break
                q.append(c)
            else:
                j = int(np.ravel_multi_index(tuple(q), shape))
                assert j != i
                edges.add((min(i, j), max(i, j)))
    return sorted(edges)


def _trim(off, dists):
    n = off.shape[0]
    for k, s in enumerate(dists):
        assert np.all(off[n - s:, k] == 0.0)                          # zeros in every ignored tail
    return [off[:n - s, k].copy() for k, s in enumerate(dists)]


_LAP = {}


def _stencil(shape, kind):
    """kappa L of the grid graph from the package's builder: (deg, trimmed couplings, distances); computed once per (shape, kind), read-only."""
    key = (tuple(shape), kind)
    if key not in _LAP:
        deg, off, dists = L.grid_laplacian(shape, KAPPA, **_STENCILS[kind])
        assert off.flags.f_contiguous and off.shape == (len(deg), len(dists))
        offs = _trim(off, dists)
        deg.setflags(write=False)
        for e in offs:
            e.setflags(write=False)
        _LAP[key] = (deg, offs, dists)
    return _LAP[key]


# ---- 1. the builders ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,periodic,corners,dists", [
    ((6, 7, 8), False, True, (1, 7, 8, 9, 47, 48, 49, 55, 56, 57, 63, 64, 65)),
    ((30, 50), True, False, (1, 49, 50, 1450)),
    ((12, 13, 14), True, False, (1, 13, 14, 168, 182, 2002)),
    ((18, 50), True, True, 10),
    ((4, 5, 6), (True, False, True), False, (1, 5, 6, 30, 90)),
    ((3, 3), True, True, (1, 2, 3, 4, 5, 6, 7, 8)),
    ((5, 4), (True, False), True, None), ((2, 3, 2), False, True, None), ((1, 7), (False, True), False, (1, 6))])
def test_grid_laplacian_with_periodic_axes_and_corner_neighbours(shape, periodic, corners, dists):
    n = int(np.prod(shape))
    deg, off, ds = L.grid_laplacian(shape, KAPPA, periodic=periodic, corners=corners)
    if isinstance(dists, int):
        assert len(ds) == dists
    elif dists is not None:
        assert ds == dists
    assert list(ds) == sorted(set(ds)) and 1 <= ds[0] and ds[-1] < n
    assert off.flags.f_contiguous and off.shape == (n, len(ds)) and deg.shape == (n,)
    offs = _trim(off, ds)
    edges = _edges(shape, periodic, corners)
    assert sorted(set(j - i for i, j in edges)) == list(ds)
    # the same matrix, entry by entry: -kappa on every edge, nothing else; the diagonal kappa deg
    ref_deg = np.zeros(n)
    ref_off = np.zeros((n, len(ds)))
    for i, j in edges:
        ref_deg[i] += KAPPA
        ref_deg[j] += KAPPA
        ref_off[i, ds.index(j - i)] -= KAPPA
    assert np.array_equal(off, ref_off)
    assert np.abs(deg - ref_deg).max() <= 1e-14 * ref_deg.max()
    # ... and the quadratic form  v'Lv = sum_edges (v_i - v_j)^2
    v = synth.hash_vector(30, n)
    ei, ej = np.array(edges).T
    quad = KAPPA * np.sum((v[ei] - v[ej]) ** 2)
    assert abs(v @ _apply(v, deg, offs, ds) - quad) <= 1e-12 * quad
    if corners and min(shape) >= 3:
        assert abs(deg.max() - KAPPA * (3 ** len(shape) - 1)) <= 1e-12           # 8 / 26 neighbours inside


def test_grid_laplacian_refusals_and_defaults():
    with pytest.raises(ValueError, match=r"\b\d\d distinct"):                     # a periodic 3-D grid with corners: the count is named
        L.grid_laplacian((5, 6, 7), 1.0, periodic=True, corners=True)
    with pytest.raises(AssertionError):
        L.grid_laplacian((2, 5), 1.0, periodic=True)                               # the wrap on 2 points would duplicate the edge
    with pytest.raises(AssertionError):
        L.grid_laplacian((4, 2, 5), 1.0, periodic=(False, True, False), corners=True)
    L.grid_laplacian((2, 5), 1.0, periodic=(False, True))                          # (the axis of length 2 is not the periodic one)
    # the default flags: today's arrays (the axis-by-axis construction, spelled out here), array for array
    for shape in ((30, 50), (12, 13, 14), (1, 9), (5, 1, 4)):
        n = int(np.prod(shape))
        deg, off, ds = L.grid_laplacian(shape, KAPPA)
        deg2, off2, ds2 = L.grid_laplacian(shape, KAPPA, periodic=False, corners=False)
        assert ds == ds2 and np.array_equal(deg, deg2) and np.array_equal(off, off2)
        strides = [int(np.prod(shape[ax + 1:])) for ax in range(len(shape))]
        want = tuple(sorted(st for st, s in zip(strides, shape) if s > 1))
        assert ds == want and off.shape == (n, len(want)) and off.flags.f_contiguous
        idx = np.arange(n).reshape(shape)
        rdeg = np.zeros(n)
        for st, (ax, s) in zip(strides, enumerate(shape)):
            if s > 1:
                lo = np.take(idx, np.arange(s - 1), axis=ax).ravel()
                col = np.zeros(n)
                col[lo] = -KAPPA
                assert np.array_equal(off[:, ds.index(st)], col)
                rdeg[lo] += KAPPA
                rdeg[lo + st] += KAPPA
        assert np.array_equal(deg, rdeg)


def test_graph_diagonals():
    n = 40
    i = np.array([0, 0, 3, 3, 10, 38, 0])
    j = np.array([1, 5, 4, 8, 39, 39, 5])                             # distances 1, 5, 1, 5, 29, 1 and the edge (0, 5) a second time
    w = np.array([1.0, 2.0, -3.0, 0.5, 4.0, 7.0, 0.25])
    diag, off, ds = L.graph_diagonals(n, i, j, w)
    assert ds == (1, 5, 29) and off.shape == (n, 3) and off.flags.f_contiguous
    A = np.zeros((n, n))
    for a, b, ww in zip(i, j, w):
        A[a, a] += ww
        A[b, b] += ww
        A[a, b] -= ww
        A[b, a] -= ww
    assert np.allclose(_dense(diag, _trim(off, ds), ds), A, rtol=0, atol=1e-15)
    v = synth.hash_vector(30, n)
    assert abs(v @ A @ v - np.sum(w * (v[i] - v[j]) ** 2)) <= 1e-13
    d1, o1, s1 = L.graph_diagonals(5, [0, 1], [1, 4], 2.0)            # a scalar weight
    assert s1 == (1, 3) and np.array_equal(d1, [2.0, 4.0, 0.0, 0.0, 2.0]) and o1[0, 0] == -2.0 and o1[1, 1] == -2.0 and np.count_nonzero(o1) == 2
    with pytest.raises(ValueError, match="14"):
        L.graph_diagonals(20, np.zeros(14, dtype=int), np.arange(1, 15), 1.0)
    L.graph_diagonals(20, np.zeros(13, dtype=int), np.arange(1, 14), 1.0)
    with pytest.raises(AssertionError):
        L.graph_diagonals(5, [2], [1], 1.0)                           # i < j


# ---- 2. the product ----------------------------------------------------------------------------------------------------------------------
_FIB = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 2047, 2100)           # below and beyond a 2048-row tile
_DIST_SETS = [(1, 3, 55, 2047, 2100), (1, 2, 5, 13, 89, 144, 2047, 2100), _FIB, (2048, 2049, 2050, 2051, 2052)]


@pytest.mark.parametrize("dists", _DIST_SETS, ids=lambda d: f"K{len(d)}-{d[0]}")
def test_stencil_product(dev_ctx, dists):
    ctx = dev_ctx
    assert len(dists) > 4
    for n in (2200, 4097, 6300):
        a = 4.0 * synth.hash_vector(3, n) + 5.0
        offs = [0.8 / (k + 1) * synth.hash_vector(16 + k, n)[:n - s] for k, s in enumerate(dists)]
        assert all(np.any(e > 0) and np.any(e < 0) for e in offs)
        vh = synth.hash_vector(7, n)
        A = _operator(ctx, a, offs, dists, a0=0.25)                  # (ignored tails and one extra column poisoned)
        assert A._wide
        out = ctx.vector(n)
        A.mul_(out, ctx.vector(n, vh))
        ref = _apply(vh, a, offs, dists)
        err = np.abs(out.download() - ref).max()
        print(f"[stencil product] K={len(dists)} n={n}: {err:.1e}")
        assert err <= 1e-14 * max(1.0, np.abs(ref).max()), n
        out.upload(np.ones(n))
        A.mul_(out, ctx.vector(n, vh), 2.0, -1.0)                   # mul!(dest, A, v, alpha, beta)
        assert np.abs(out.download() - (2.0 * ref - 1.0)).max() <= 1e-13 * max(1.0, np.abs(ref).max()), n
        # stacked pair: the couplings on the x half, the y half diagonal, the gap left at zero
        ay = synth.hash_vector(16, n)
        vs = synth.hash_vector(8, 2 * n)
        As = _operator(ctx, a, offs, dists, a0=0.25, ay=ay)
        outs = L.StackedVector(ctx, n)
        As.mul_(outs, L.StackedVector(ctx, n).upload2(vs))
        refs = _DiagsRef(a, offs, dists, ay)._op(vs)
        assert np.abs(outs.download2() - refs).max() <= 1e-14 * max(1.0, np.abs(refs).max()), n
        assert not np.any(outs.download(outs.hs - n, n))


# ---- 3. solves on one pass ---------------------------------------------------------------------------------------------------------------
def _case_operator(shape, kind):
    """(a, offs, dists, dominant): kappa L + a on the stencil `kind`, or ('rand27') couplings 1.2 hash_vector(15 + k) of both signs on the
    27-point pattern's nonzeros under a = 4 hash_vector(3) + 14 -- positive definite, not diagonally dominant."""
    n = int(np.prod(shape))
    if kind == "rand27":
        _, pat, dists = _stencil(shape, "27")
        offs = [np.where(p != 0.0, 1.2 * synth.hash_vector(15 + k, n)[:n - s], 0.0) for k, (p, s) in enumerate(zip(pat, dists))]
        return 4.0 * synth.hash_vector(3, n) + 14.0, offs, dists, False
    deg, offs, dists = _stencil(shape, kind)
    return deg + 0.05 + 0.5 * synth.hash_vector(3, n) ** 2, offs, dists, True


_ORACLE = {}


def _oracle_solve(key, Aref, Uh, bh, c0, m):
    """The oracle's side of a count comparison: `_conditioned_tol`'s (tol, count, margins) and the solve at that tolerance (x, lambda, count, nr).
    With a key it is computed once and shared between the emulator and the GPU runs of a case (read-only)."""
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


# (grid, stencil, m, factored, the oracle's count at tol = 1e-10 for c = 0; None: the factored basis is this file's own choice)
_CASES = [((6, 7, 8), "27", 6, False, 51), ((12, 13, 14), "27", 130, False, 59), ((3, 4, 700), "27", 33, False, 145),
          ((30, 50), "per", 6, False, 75), ((12, 13, 14), "per", 33, False, 66), ((5, 6, 420), "per", 6, False, 96),
          ((18, 50), "percorn", 33, False, 64),
          ((6, 7, 8), "rand27", 6, False, 22), ((12, 13, 14), "rand27", 33, False, 24),
          ((12, 13, 14), "27", 130, True, None), ((18, 50), "percorn", 33, True, None)]


@pytest.mark.parametrize("shape,kind,m,factored,count", _CASES)
def test_projcg_with_a_wide_stencil_on_one_pass(dev_ctx, shape, kind, m, factored, count):
    """'rand27' is this file's choice of data (dense check with numpy, not the code under test): 94 and 979 negative Gram weights,
    lambda_min = 5.74 and 5.75; the oracle takes 22 and 24 iterations."""
    ctx = dev_ctx
    n = int(np.prod(shape))
    a, offs, dists, dominant = _case_operator(shape, kind)
    assert len(dists) == {"27": 13, "rand27": 13, "percorn": 10, "per": 2 * len(shape)}[kind]
    if not dominant:
        cw = a.copy()
        for e, s in zip(offs, dists):
            cw[:n - s] -= np.abs(e)
            cw[s:] -= np.abs(e)
        lmin = np.linalg.eigvalsh(_dense(a, offs, dists))[0]
        print(f"[stencil] {shape} {np.count_nonzero(cw < 0)} negative Gram weights, lambda_min = {lmin:.3f}")
        assert np.any(cw < 0)                                        # some Gram weight c_i is negative: the extra pass runs
        assert lmin > 0.05
    U, Uh = _basis(ctx, n, m, factored)
    A = _operator(ctx, a, offs, dists)
    Aref = _DiagsRef(a, offs, dists)
    bh = synth.hash_vector(4, n)
    b = ctx.vector(n, bh)
    work = L.ProjCGWork(ctx, n, m)
    for ch in (None, np.linspace(-1, 1, m)):
        c0 = np.zeros(m) if ch is None else ch
        key = None if factored else (shape, kind, m, ch is None)      # (the factored basis comes from the device's own ksvd_)
        tol, i_base, up, down, x0, l0, i0, nr0 = _oracle_solve(key, Aref, Uh, bh, c0, m)
        print(f"[stencil] {shape} {kind} m={m} factored={factored} c={'0' if ch is None else 'given'}: oracle {i_base} iterations at 1e-10, "
              f"tol {tol:.3e}, margins {up:.2f} / {down:.2f}")
        if ch is None and count is not None:
            assert i_base == count
        assert up >= 1.1 and down >= 1.1
        assert i0 == i_base
        x, lam = ctx.vector(n), ctx.vector(m)
        i1, nr1 = L.projcg_(x, lam, A, U, b, None if ch is None else ctx.vector(m, ch), tol=tol, work=work)
        dx = np.linalg.norm(x.download() - x0) / np.linalg.norm(x0)
        dl = np.abs(lam.download() - l0).max()
        print(f"[stencil]   iterations {i1} (oracle {i0}), nr {nr1:.6e} ({nr0:.6e}), x {dx:.1e}, lambda {dl:.1e}")
        assert i1 == i0 and i1 > 3 and nr1 == pytest.approx(nr0, rel=1e-5)
        assert dx <= 1e-10
        assert dl <= 1e-10
    # the iteration limit (src/projcg.jl:71)
    x0, l0 = np.zeros(n), np.zeros(m)
    i0, nr0 = R.projcg_(x0, l0, Aref, Uh, bh, np.zeros(m), tol=1e-30, maxit=5)
    x, lam = ctx.vector(n), ctx.vector(m)
    i1, nr1 = L.projcg_(x, lam, A, U, b, None, tol=1e-30, maxit=5, work=work)
    assert (i1, i0) == (5, 5) and nr1 == pytest.approx(nr0, rel=1e-9)
    assert np.linalg.norm(x.download() - x0) <= 1e-12 * np.linalg.norm(x0)
    # negative curvature (src/projcg.jl:77-82)
    x0, l0 = np.zeros(n), np.zeros(m)
    i0, nr0 = R.projcg_(x0, l0, _DiagsRef(-a, offs, dists), Uh, bh, np.zeros(m), tol=1e-10)
    x, lam = ctx.vector(n), ctx.vector(m)
    i1, nr1 = L.projcg_(x, lam, _operator(ctx, -a, offs, dists), U, b, None, tol=1e-10, work=work)
    assert (i1, nr1) == (i0, nr0) and math.isinf(nr1)
    assert np.linalg.norm(x.download() - x0) <= 1e-10 and np.all(np.isnan(lam.download()))


# ---- 4. agreement with what exists -------------------------------------------------------------------------------------------------------
def _solve_c(ctx, entry, A, K, U, b, m, tol, maxit=10_000, flags=1, c=None):
    """One of the two C solvers on a plain basis: (rc, iterations, nr, x, lambda) -- new vectors and work space per call."""
    n = b.n
    x, lam, Av = ctx.vector(n), ctx.vector(m), ctx.vector(n)
    work = L.ProjCGWork(ctx, n, m)
    it, nr = _capi.c_i64(), C.c_double()
    u_c, w_c = U._c(), work._c()
    rc = getattr(ctx.L, entry)(ctx.h, x.h, lam.h, A.a0, A._dg_h(), A.off.h, K, A._dist_c, Av.h, C.byref(u_c), b.h, None if c is None else c.h,
                               float(tol), int(maxit), n, flags, C.byref(w_c), C.byref(it), C.byref(nr))
    return rc, it.value, nr.value, x.download(), lam.download()


@pytest.mark.parametrize("dists", [(1, 50), (1, 49, 50, 51)], ids=lambda d: "-".join(map(str, d)))
def test_up_to_four_distances_return_the_bits_of_the_diags_entries(dev_ctx, dists):
    ctx = dev_ctx
    shape, m = (40, 50), 33
    n = 2000
    a = 4.0 * synth.hash_vector(3, n) + 9.0
    offs = [1.5 / (k + 1) * synth.hash_vector(15 + k, n)[:n - s] for k, s in enumerate(dists)]
    A = _operator(ctx, a, offs, dists, a0=0.5)
    assert not A._wide
    U, _ = _basis(ctx, n, m, False)
    b = ctx.vector(n, synth.hash_vector(4, n))
    cv = ctx.vector(m, np.linspace(-1, 1, m))
    K = len(dists)
    for c in (None, cv):
        old = _solve_c(ctx, "lfpsqp_projcg_diags", A, K, U, b, m, 1e-10, c=c)
        new = _solve_c(ctx, "lfpsqp_projcg_stencil", A, K, U, b, m, 1e-10, c=c)
        assert old[0] == 0 and new[0] == 0 and old[1] > 3
        assert new[1] == old[1] and new[2] == old[2]
        assert np.array_equal(new[3], old[3]) and np.array_equal(new[4], old[4])
    v = ctx.vector(n, synth.hash_vector(7, n))
    o1, o2 = ctx.vector(n), ctx.vector(n)
    assert ctx.L.lfpsqp_diags_mul(ctx.h, A.a0, A._dg_h(), A.off.h, K, A._dist_c, v.h, o1.h) == 0
    assert ctx.L.lfpsqp_stencil_mul(ctx.h, A.a0, A._dg_h(), A.off.h, K, A._dist_c, v.h, o2.h) == 0
    assert np.array_equal(o1.download(), o2.download()) and np.any(o1.download())


def test_callback_path_agrees_with_the_one_pass_solve_at_thirteen_distances(dev_ctx):
    ctx = dev_ctx
    shape, m = (6, 7, 8), 6
    n = 336
    a, offs, dists, _ = _case_operator(shape, "27")
    A = _operator(ctx, a, offs, dists)
    U, Uh = _basis(ctx, n, m, False)
    bh = synth.hash_vector(4, n)
    b = ctx.vector(n, bh)
    for ch in (None, np.linspace(-1, 1, m)):
        tol, i_base, up, down = _conditioned_tol(_DiagsRef(a, offs, dists), Uh, bh, np.zeros(m) if ch is None else ch, m)
        assert up >= 1.1 and down >= 1.1
        res = []
        for fused in (True, False):
            A.fused = fused
            x, lam = ctx.vector(n), ctx.vector(m)
            it, nr = L.projcg_(x, lam, A, U, b, None if ch is None else ctx.vector(m, ch), tol=tol, work=L.ProjCGWork(ctx, n, m))
            res.append((it, x.download(), lam.download()))
        A.fused = True
        assert res[0][0] == res[1][0] == i_base
        assert np.linalg.norm(res[0][1] - res[1][1]) <= 1e-10 * np.linalg.norm(res[0][1])
        assert np.abs(res[0][2] - res[1][2]).max() <= 1e-10


# ---- 5. bounds ---------------------------------------------------------------------------------------------------------------------------
def _solve_stacked_c(ctx, A, P, b, n, m, tol, maxit=None):
    """lfpsqp_projcg_stencil itself over a stacked basis (no fall-back): rc, iterations, nr, x, lambda."""
    x, lam = L.StackedVector(ctx, n), ctx.vector(n + m)
    work = L.ProjCGWork(ctx, 0, m, stacked_N=n)
    Av = L.StackedVector(ctx, n)
    it, nr = _capi.c_i64(), C.c_double()
    u_c, w_c = P._c(), work._c()
    rc = ctx.L.lfpsqp_projcg_stencil(ctx.h, x.h, lam.h, A.a0, A.dg.h, A.off.h, len(A.dists), A._dist_c, Av.h, C.byref(u_c), b.h, None, float(tol),
                                     int(2 * n + m if maxit is None else maxit), 2 * n, 1, C.byref(w_c), C.byref(it), C.byref(nr))
    return rc, it.value, nr.value, x, lam


@pytest.mark.parametrize("shape,kind,m,factored", [((6, 7, 8), "27", 16, False), ((12, 13, 14), "per", 33, False), ((6, 7, 8), "27", 16, True)])
def test_stacked_stencil_solver_follows_the_oracle(dev_ctx, shape, kind, m, factored):
    """Four-way bounds: lfpsqp_projcg_stencil over a stacked basis against the oracle's projcg! with the augmented map blockdiag(T, diag(ay))."""
    ctx = dev_ctx
    n = int(np.prod(shape))
    P, P0, _, rank = _stacked_problem(ctx, n, m, factored)
    assert rank == m
    ax, offs, dists, _ = _case_operator(shape, kind)
    ay = 0.5 + synth.hash_vector(16, n) ** 2
    A = _operator(ctx, ax, offs, dists, ay=ay)
    assert A._wide
    Aref = _DiagsRef(ax, offs, dists, ay)
    bh = synth.hash_vector(4, 2 * n)
    tmp = np.zeros(n + m)
    R.mul_(tmp, R.adj(P0), bh)
    R.mul_(bh, P0, tmp, -1.0, 1.0)                                      # a right-hand side in the tangent space, like optimize's d
    b = L.StackedVector(ctx, n).upload2(bh)
    tol_c, i_base, up, down = _conditioned_tol(Aref, P0, bh, np.zeros(n + m), n + m)
    print(f"[stacked stencil] {shape} {kind} m={m} factored={factored}: oracle {i_base} iterations at 1e-10, tol {tol_c:.3e}, margins {up:.2f} / {down:.2f}")
    assert up >= 1.1 and down >= 1.1
    for tol, maxit in ((tol_c, None), (1e-300, 5)):
        x0, l0 = np.zeros(2 * n), np.zeros(n + m)
        i0, nr0 = R.projcg_(x0, l0, Aref, P0, bh, np.zeros(n + m), tol=tol, maxit=maxit)
        rc, i1, nr1, x, lam = _solve_stacked_c(ctx, A, P, b, n, m, tol, maxit)
        assert rc == 0
        xd, ld = x.download2(), lam.download()
        dx_ = np.linalg.norm(xd - x0) / np.linalg.norm(x0)
        dl_ = np.abs(ld - l0).max() / np.abs(l0).max()
        print(f"[stacked stencil]   maxit={maxit}: iterations {i1} (oracle {i0}), nr {nr1:.6e} ({nr0:.6e}), x {dx_:.1e}, lambda {dl_:.1e}")
        assert i1 == i0 and (maxit is not None or (i1 == i_base and i1 > 3))
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
    i0, nr0 = R.projcg_(x0, l0, _DiagsRef(-ax, offs, dists, ay), P0, bh, np.zeros(n + m), tol=1e-10)
    rc, i1, nr1, x, lam = _solve_stacked_c(ctx, _operator(ctx, -ax, offs, dists, ay=ay), P, b, n, m, 1e-10)
    assert rc == 0 and (i1, nr1) == (i0, nr0) and math.isinf(nr1)
    assert np.all(np.isnan(lam.download()))


# ---- 6. optimize -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,flags,entry", [((6, 7, 8), dict(corners=True), "lfpsqp_projcg_stencil"),
                                               ((10, 12), dict(periodic=True), "lfpsqp_projcg_diags")], ids=["27-point", "periodic"])
def test_grid_objective_with_wide_stencils_follows_the_oracle(dev_ctx, shape, flags, entry):
    """GridSeparableLinear(..., corners / periodic) with ball and box through `optimize`: every truncated-Newton solve runs a DiagonalsOperator
    from the tangent step's state on the one-pass entry (13 distances: lfpsqp_projcg_stencil; the periodic 5-point stencil has 4 and stays on
    lfpsqp_projcg_diags), and the trajectory is the oracle's with hess_lag_vec! a matrix-free map over graph_diagonals' arrays.  The oracle is
    run a second time from one ulp away, as in tests/test_projcg_diags.py."""
    ctx = dev_ctx
    n, m = int(np.prod(shape)), 4
    maxiter, kind = 8, 1
    per = (bool(flags.get("periodic", False)),) * len(shape)
    ei, ej = np.array(_edges(shape, per[0], bool(flags.get("corners", False)))).T
    deg, off, dists = L.graph_diagonals(n, ei, ej, KAPPA)
    offs = _trim(off, dists)
    assert len(dists) == (13 if "corners" in flags else 4)

    def pen(v):
        return _apply(v, deg, offs, dists)
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
    P = L.GridSeparableLinear(ctx, shape, m, ctx.matrix(n + 1, m + 1).hash_fill(1, 0, n, 1.0, n, m), P0.eq.b, kind, a, c, kappa=KAPPA,
                              R2=P0.R2, xl=P0.xl, xu=P0.xu, **flags)
    assert P.diagonals[0] == dists and P.diagonals[1].m == len(dists)
    assert not np.any(P.diagonals[1].download()[n:])                 # the slack row has no couplings
    OPT = sys.modules["lfpsqp_jl_amd.optimize"]
    seen, rcs, orig = [], [], OPT.projcg_
    c_entry = getattr(ctx.L, entry)

    def spy(*args, **kw):
        seen.append((type(args[2]).__name__, bool(kw.get("start_given"))))
        return orig(*args, **kw)

    def c_spy(*args):
        rc = c_entry(*args)
        rcs.append(rc)
        return rc
    OPT.projcg_ = spy
    setattr(ctx.L, entry, c_spy)
    try:
        x, obj, lam, ti = P.optimize(x0, L.LFPSQPParams(disp=L.DisplayOption.off, **par), trace=tr)
    finally:
        OPT.projcg_ = orig
        setattr(ctx.L, entry, c_entry)
    assert seen and all(s == ("DiagonalsOperator", True) for s in seen)
    assert len(rcs) == len(seen) and all(rc == 0 for rc in rcs)
    assert ti.iter == tir.iter and ti.condition.name == tir.condition.name
    print(f"[grid {shape} {flags}] Newton-system iterations", [t.get('tn_iter') for t in tr0])
    assert any((t.get('tn_iter') or 0) > 3 for t in tr0)
    rtol = max(1e-10, 10.0 * max(sens))
    _note(f"grid objective {shape} {flags}: the oracle's one-ulp sensitivity {max(sens):.1e}")
    assert max(sens) <= 1e-12                                        # (the comparison below is at 1e-10, not at the oracle's own spread)
    assert _compare_traces(tr, tr0, rtol=rtol) is None
    assert abs(obj[-1] - objr[-1]) <= 1e-11 * abs(objr[-1])
    assert np.linalg.norm(x - xr) <= 1e-10 * np.linalg.norm(xr)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def _dist_array(*d):
    return (_capi.c_i64 * max(len(d), 1))(*d)


def test_stencil_entries_refuse_what_has_no_one_pass_form(dev_ctx):
    ctx = dev_ctx
    n, m = 900, 8
    dists = tuple(range(1, 28, 2))                                  # 14 distances; the first 13 make the operator
    a = 5.0 + synth.hash_vector(3, n)
    offs = [0.1 * synth.hash_vector(15 + k, n)[:n - s] for k, s in enumerate(dists)]
    off14 = _off_matrix(ctx, n, offs, dists)
    dg = ctx.vector(n, a)
    b = ctx.vector(n, synth.hash_vector(4, n))
    A = L.DiagonalsOperator(0.0, dg, off14, dists[:13])
    with pytest.raises(ValueError, match="14"):
        L.DiagonalsOperator(0.0, dg, off14, dists)
    bad = [(0, _dist_array(1)), (14, _dist_array(*dists)), (5, _dist_array(1, 3, 9, 7, 11)), (5, _dist_array(1, 3, 7, 7, 11)),
           (5, _dist_array(0, 3, 5, 7, 11)), (5, _dist_array(-1, 3, 5, 7, 11)), (5, _dist_array(1, 3, 5, 7, n)), (1, _dist_array(n + 5)), (5, None)]
    for view in (False, True):
        Uh, _ = np.linalg.qr(synth.hash_matrix(1, n, m))
        Zd = ctx.matrix(n, m, np.asfortranarray(Uh))
        U = L.DeviceBasis(Zd.view(ctx.vector(n, np.ones(n))) if view else Zd)
        x, lam, Av = ctx.vector(n), ctx.vector(m), ctx.vector(n)
        work = L.ProjCGWork(ctx, n, m)
        it, nr = _capi.c_i64(), C.c_double()
        u_c, w_c = U._c(), work._c()

        def solve(K, dist, flags=1, offh=off14.h):
            return ctx.L.lfpsqp_projcg_stencil(ctx.h, x.h, lam.h, 0.0, dg.h, offh, K, dist, Av.h, C.byref(u_c), b.h, None, 1e-10, 100, n, flags,
                                               C.byref(w_c), C.byref(it), C.byref(nr))
        for K, dist in bad:
            assert solve(K, dist) == -1, (K, None if dist is None else list(dist))
            assert ctx.L.lfpsqp_stencil_mul(ctx.h, 0.0, dg.h, off14.h, K, dist, b.h, Av.h) == -1, (K, None if dist is None else list(dist))
        if view:
            assert solve(13, A._dist_c) == -5                       # LFPSQP_ERR_UNSUPPORTED: a matrix view as basis
            continue
        assert solve(13, A._dist_c, flags=1 | L.projcg.RESUME) == -1
        assert solve(13, A._dist_c, flags=1 | L.projcg.START_PROJECTED) == -1
        assert solve(13, A._dist_c) == 0 and it.value > 3
        offv = off14.view(ctx.vector(n, np.ones(n)))                # a view as the couplings
        assert solve(13, A._dist_c, offh=offv.h) == -1
        assert ctx.L.lfpsqp_stencil_mul(ctx.h, 0.0, dg.h, offv.h, 13, A._dist_c, b.h, Av.h) == -1
        assert ctx.L.lfpsqp_stencil_mul(ctx.h, 0.0, dg.h, off14.h, 13, A._dist_c, b.h, Av.h) == 0


def test_stencil_entries_refuse_row_shards(emu_lib):
    """A communicator (the row-shard case): the one-pass solve and the product answer LFPSQP_ERR_UNSUPPORTED; projcg_ raises."""
    ctx = L.Context(0, emu_lib)
    try:
        ctx.comm_init_callback(0, 1, lambda ptr, count, op, stream: 0)
        shape, m = (6, 7, 8), 8
        n = 336
        a, offs, dists, _ = _case_operator(shape, "27")
        A = _operator(ctx, a, offs, dists)
        Uh, _ = np.linalg.qr(synth.hash_matrix(1, n, m))
        U = L.DeviceBasis(ctx.matrix(n, m, np.asfortranarray(Uh)))
        b, x, lam, Av = ctx.vector(n, synth.hash_vector(4, n)), ctx.vector(n), ctx.vector(m), ctx.vector(n)
        work = L.ProjCGWork(ctx, n, m)
        it, nr = _capi.c_i64(), C.c_double()
        u_c, w_c = U._c(), work._c()
        rc = ctx.L.lfpsqp_projcg_stencil(ctx.h, x.h, lam.h, 0.0, A.dg.h, A.off.h, 13, A._dist_c, Av.h, C.byref(u_c), b.h, None, 1e-10, 100, n, 1,
                                         C.byref(w_c), C.byref(it), C.byref(nr))
        assert rc == -5
        assert ctx.L.lfpsqp_stencil_mul(ctx.h, 0.0, A.dg.h, A.off.h, 13, A._dist_c, b.h, Av.h) == -5
        with pytest.raises(L.LfpsqpError):
            L.projcg_(x, lam, A, U, b, None, tol=1e-10, work=work)
    finally:
        ctx.close()


# ---- 8. a size at which a workgroup of the vector launches takes several rounds --------------------------------------------------------------
@pytest.mark.gpu
def test_stencil_at_a_size_of_several_rounds(gpu_lib):
    """(41, 41, 42), n = 70602, m = 16, the 27-point stencil: the product against numpy, a solve capped at 30 iterations against the oracle."""
    ctx = L.Context(0, gpu_lib)
    try:
        shape, m = (41, 41, 42), 16
        n = 70602
        a, offs, dists, _ = _case_operator(shape, "27")
        assert len(dists) == 13 and dists[-1] == 41 * 42 + 42 + 1
        A = _operator(ctx, a, offs, dists)
        vh = synth.hash_vector(7, n)
        out = ctx.vector(n)
        A.mul_(out, ctx.vector(n, vh))
        ref = _apply(vh, a, offs, dists)
        assert np.abs(out.download() - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max())
        U, Uh = _basis(ctx, n, m, False)
        bh = synth.hash_vector(4, n)
        x0, l0 = np.zeros(n), np.zeros(m)
        i0, nr0 = R.projcg_(x0, l0, _DiagsRef(a, offs, dists), Uh, bh, np.zeros(m), tol=1e-300, maxit=30)
        x, lam = ctx.vector(n), ctx.vector(m)
        i1, nr1 = L.projcg_(x, lam, A, U, ctx.vector(n, bh), None, tol=1e-300, maxit=30, work=L.ProjCGWork(ctx, n, m))
        dx = np.linalg.norm(x.download() - x0) / np.linalg.norm(x0)
        dl = np.abs(lam.download() - l0).max()
        print(f"[stencil 70602] iterations {i1} (oracle {i0}), nr {nr1:.6e} ({nr0:.6e}), x {dx:.1e}, lambda {dl:.1e}")
        assert (i1, i0) == (30, 30) and nr1 == pytest.approx(nr0, rel=1e-5)
        assert dx <= 1e-10 and dl <= 1e-10
    finally:
        ctx.close()
