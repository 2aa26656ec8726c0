"""projcg! with a GRID-STENCIL Hessian -- a diagonal plus up to four off-diagonals at arbitrary distances -- on the one-pass iteration
(lfpsqp_projcg_diags).

A smoothness / diffusion term on a 2-D or 3-D field stored in row-major order couples point i with i + 1, i + nx (and i + nx ny, or
i + nx -+ 1 for the 9-point stencil): off-diagonals FAR from the main one, which the banded entry (distances 1 .. 4) refuses.  The diagonals entry
keeps ONE pass over the basis per iteration: the pass is the tridiagonal one, two vector kernels before it store A d and gather the neighbours'
part of A rr at the shifted rows, and U'A U takes one shifted Gram pass per off-diagonal with the distance as a run-time argument
(include/lfpsqp_hip.h).  Checked here against numpy and the oracle's projcg! with the same operator as a matrix-free map: the product (plain,
stacked, ignored entries poisoned), counts / iterates / multipliers on 2-D, 3-D and 9-point grids with distances below and beyond a 2048-row
tile, dominant and non-dominant couplings, c != 0, the iteration limit, negative curvature, materialised and factored bases, the callback path,
distances (1, 2) against the banded entry, the stacked form under four-way bounds, GridSeparableLinear through `optimize`, and the refusals.

EXIT CONDITION of the count comparisons.  At tol = 1e-10 the oracle's residual norm one iteration before its exit can lie within a few per cent
of the tolerance (1.04 tol on the 30 x 50 grid), and "equal counts" would test the last bits of a norm rather than the kernels.  Every solve that
compares counts therefore takes as tolerance the geometric mean of the oracle's last two residual norms (the oracle run to the base tolerance
for its count i, once more with maxit = i - 1 for the norm before), and asserts ON THE ORACLE ALONE, before the device is looked at, that both
norms are at least a factor 1.1 away from it (`_conditioned_tol`)."""
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


def _apply(v, a, offs, dists):
    """(A v) = a v + sum_k (off_k[i-s_k] v_{i-s_k} + off_k[i] v_{i+s_k}) over len(a) rows; offs[k] holds the n - s_k used couplings."""
    n = len(a)
    out = a * v[:n]
    for e, s in zip(offs, dists):
        out[:n - s] += e * v[s:n]
        out[s:n] += e * v[:n - s]
    return out


class _DiagsRef:
    def __init__(self, a, offs, dists, ay=None):
        self.a, self.offs, self.dists, self.ay = a, offs, dists, ay

    def _op(self, v):
        if self.ay is None:
            return _apply(v, self.a, self.offs, self.dists)
        n = len(self.a)
        return np.concatenate([_apply(v[:n], self.a, self.offs, self.dists), self.ay * v[n:]])

    def mul_(self, dest, v, al=None, be=None):
        t = self._op(v)
        dest[:] = t if al is None else al * t + be * dest
        return dest

    def adjoint(self):
        return self


def _off_matrix(ctx, n, offs, dists, extra_cols=0):
    """n x (K + extra) device matrix, column k = off_k with its ignored tail (rows i + s_k >= n) and any extra column poisoned."""
    K = len(offs)
    M = np.full((n, K + extra_cols), POISON, order='F')
    for k, e in enumerate(offs):
        assert len(e) == n - dists[k]
        M[:len(e), k] = e
    return ctx.matrix(n, K + extra_cols, M)


def _operator(ctx, a, offs, dists, a0=0.0, ay=None):
    n = len(a)
    if ay is None:
        dg = ctx.vector(n, a - a0)
    else:
        dg = L.StackedVector(ctx, n).upload2(np.concatenate([a, ay]) - a0)
    return L.DiagonalsOperator(a0, dg, _off_matrix(ctx, n, offs, dists, extra_cols=1), dists)


def _rand_offs(n, dists, scale, seed=15):
    return [scale * synth.hash_vector(seed + k, n)[:n - s] for k, s in enumerate(dists)]


def _dense(a, offs, dists):
    A = np.diag(a)
    for e, s in zip(offs, dists):
        A += np.diag(e, s) + np.diag(e, -s)
    return A


def _laplacian(shape, kappa):
    """kappa L of the grid graph from the package's own builder, checked against np.diff along each axis: (deg, trimmed couplings, distances)."""
    deg, off, dists = L.grid_laplacian(shape, kappa)
    n = int(np.prod(shape))
    offs = [off[:n - s, k].copy() for k, s in enumerate(dists)]
    v = synth.hash_vector(30, n)
    ref = np.zeros(shape)
    V = v.reshape(shape)
    for ax in range(len(shape)):
        if shape[ax] > 1:
            pad = [(0, 0)] * len(shape)
            pad[ax] = (1, 1)
            ref -= kappa * np.diff(np.pad(np.diff(V, axis=ax), pad), axis=ax)
    assert np.abs(_apply(v, deg, offs, dists) - ref.ravel()).max() <= 1e-13 * max(1.0, np.abs(ref).max())
    for k, s in enumerate(dists):
        assert np.all(off[n - s:, k] == 0.0)
    return deg, offs, dists


def _laplacian9(ny, nx, kappa):
    """kappa L of the 9-point grid graph (edges -kappa, diagonals -kappa / 2), row-major: distances (1, nx - 1, nx, nx + 1)."""
    n = ny * nx
    r, c = np.divmod(np.arange(n), nx)
    dists = (1, nx - 1, nx, nx + 1)
    full = [np.where(c < nx - 1, -kappa, 0.0),
            np.where((c > 0) & (r < ny - 1), -0.5 * kappa, 0.0),
            np.where(r < ny - 1, -kappa, 0.0),
            np.where((c < nx - 1) & (r < ny - 1), -0.5 * kappa, 0.0)]
    offs = [f[:n - s].copy() for f, s in zip(full, dists)]
    for f, s in zip(full, dists):
        assert not np.any(f[n - s:])
    deg = np.zeros(n)
    for e, s in zip(offs, dists):
        deg[:n - s] -= e
        deg[s:] -= e
    v = synth.hash_vector(30, n)
    V = v.reshape(ny, nx)
    quad = kappa * (np.sum(np.diff(V, axis=0) ** 2) + np.sum(np.diff(V, axis=1) ** 2)
                    + 0.5 * np.sum((V[1:, 1:] - V[:-1, :-1]) ** 2) + 0.5 * np.sum((V[1:, :-1] - V[:-1, 1:]) ** 2))
    assert abs(v @ _apply(v, deg, offs, dists) - quad) <= 1e-12 * quad
    return deg, offs, dists


def _conditioned_tol(Aref, Uh, bh, ch, nl, base=1e-10):
    """The tolerance of a count comparison (module docstring): (tol, the oracle's count, its margins on both sides), from the oracle alone."""
    x0, l0 = np.zeros(len(bh)), np.zeros(nl)
    i0, nr_last = R.projcg_(x0, l0, Aref, Uh, bh, ch.copy(), tol=base)
    assert i0 > 3 and math.isfinite(nr_last) and nr_last < base
    x0, l0 = np.zeros(len(bh)), np.zeros(nl)
    i_before, nr_before = R.projcg_(x0, l0, Aref, Uh, bh, ch.copy(), tol=1e-300, maxit=i0 - 1)
    assert i_before == i0 - 1 and nr_before >= base
    tol = math.sqrt(nr_last * nr_before)
    return tol, i0, nr_before / tol, tol / nr_last


_DIST_SETS = [(1,), (3,), (1, 50), (1, 2100), (1, 14, 182), (1, 49, 50, 51), (2, 2048), (7, 2047)]


@pytest.mark.parametrize("dists", _DIST_SETS, ids=lambda d: "-".join(map(str, d)))
def test_diagonals_product(dev_ctx, dists):
    ctx = dev_ctx
    sizes = [n for n in (2, 3, 17, 511, 2048, 2049, 4097, 6300) if dists[-1] < n]
    assert sizes
    for n in sizes:
        a = 4.0 * synth.hash_vector(3, n) + 5.0
        offs = [0.8 / (k + 1) * synth.hash_vector(16 + k, n)[:n - s] for k, s in enumerate(dists)]
        vh = synth.hash_vector(7, n)
        A = _operator(ctx, a, offs, dists, a0=0.25)
        out = ctx.vector(n)
        A.mul_(out, ctx.vector(n, vh))
        ref = _apply(vh, a, offs, dists)
        err = np.abs(out.download() - ref).max()
        print(f"[diags product] {dists} n={n}: {err:.1e}")
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


def _case_operator(shape, kind):
    """(a, offs, dists, dominant) of a solver case: 'lap' = kappa L + a (5- / 7-point), 'lap9' = the 9-point one, 'rand' = couplings of both signs
    on the 5-point pattern, positive definite but not diagonally dominant."""
    n = int(np.prod(shape))
    if kind == "rand":
        dists = (1, shape[-1])
        return 4.0 * synth.hash_vector(3, n) + 14.0, _rand_offs(n, dists, 3.5), dists, False
    deg, offs, dists = _laplacian9(shape[0], shape[1], 0.9) if kind == "lap9" else _laplacian(shape, 0.9)
    return deg + 0.05 + 0.5 * synth.hash_vector(3, n) ** 2, offs, dists, True


# (grid, m, operator, factored, the oracle's count at tol = 1e-10 with U = qr(hash_matrix(1)), b = hash_vector(4); None: the basis or the
# couplings are this file's own choice).  Distances below and beyond a 2048-row tile, odd and even, m from a narrow tile to past a tile width.
_CASES = [((30, 50), 6, "lap", False, 77), ((3, 2100), 6, "lap", False, 86), ((3, 2100), 33, "rand", False, None),
          ((12, 13, 14), 130, "lap", False, 64), ((64, 64), 128, "rand", False, None), ((5, 820), 300, "lap", False, 71),
          ((40, 50), 33, "lap9", False, 70), ((3, 2100), 6, "lap9", False, 87),
          ((3, 2100), 33, "lap", True, None), ((12, 13, 14), 130, "lap", True, None), ((64, 64), 128, "rand", True, None),
          ((40, 50), 33, "lap9", True, None)]


@pytest.mark.parametrize("shape,m,kind,factored,count", _CASES)
def test_projcg_with_a_diagonals_operator_on_one_pass(dev_ctx, shape, m, kind, factored, count):
    """The 'rand' cases are this file's choice of data: couplings 3.5 hash_vector(15 + k) (both signs) under a = 4 hash_vector(3) + 14.  Dense
    check of the operator (numpy, not the code under test): lambda_min = 4.45 on the 3 x 2100 grid (8 negative Gram weights) and 4.19 on the
    64 x 64 one (25); the oracle takes 28 and 29 iterations.  With a factor 3 the 3 x 2100 operator is still diagonally dominant."""
    ctx = dev_ctx
    n = int(np.prod(shape))
    a, offs, dists, dominant = _case_operator(shape, kind)
    if not dominant:
        cw = a.copy()
        for e, s in zip(offs, dists):
            cw[:n - s] -= np.abs(e)
            cw[s:] -= np.abs(e)
        assert np.any(cw < 0)                                        # some Gram weight c_i is negative: the extra pass runs
        if n <= 4096:
            lmin = np.linalg.eigvalsh(_dense(a, offs, dists))[0]
            print(f"[diags] {shape} lambda_min = {lmin:.3f}")
            assert lmin > 0.05
    U, Uh = _basis(ctx, n, m, factored)
    A = _operator(ctx, a, offs, dists)
    Aref = _DiagsRef(a, offs, dists)
    bh = synth.hash_vector(4, n)
    b = ctx.vector(n, bh)
    work = L.ProjCGWork(ctx, n, m)
    for ch in (None, np.linspace(-1, 1, m)):
        c0 = np.zeros(m) if ch is None else ch
        tol, i_base, up, down = _conditioned_tol(Aref, Uh, bh, c0, m)
        print(f"[diags] {shape} m={m} {kind} factored={factored} c={'0' if ch is None else 'given'}: oracle {i_base} iterations at 1e-10, "
              f"tol {tol:.3e}, margins {up:.2f} / {down:.2f}")
        if ch is None and count is not None:
            assert i_base == count
        assert up >= 1.1 and down >= 1.1
        x0, l0 = np.zeros(n), np.zeros(m)
        i0, nr0 = R.projcg_(x0, l0, Aref, Uh, bh, c0.copy(), tol=tol)
        assert i0 == i_base
        x, lam = ctx.vector(n), ctx.vector(m)
        i1, nr1 = L.projcg_(x, lam, A, U, b, None if ch is None else ctx.vector(m, ch), tol=tol, work=work)
        dx = np.linalg.norm(x.download() - x0) / np.linalg.norm(x0)
        dl = np.abs(lam.download() - l0).max()
        print(f"[diags]   iterations {i1} (oracle {i0}), nr {nr1:.6e} ({nr0:.6e}), x {dx:.1e}, lambda {dl:.1e}")
        assert i1 == i0 and i1 > 3 and nr1 == pytest.approx(nr0, rel=1e-5)
        assert dx <= 1e-10
        assert dl <= 1e-10
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
    i0, nr0 = R.projcg_(x0, l0, _DiagsRef(-a, offs, dists), Uh, bh, np.zeros(m), tol=1e-10)
    x, lam = ctx.vector(n), ctx.vector(m)
    i1, nr1 = L.projcg_(x, lam, _operator(ctx, -a, offs, dists), U, b, None, tol=1e-10, work=work)
    assert (i1, nr1) == (i0, nr0) and math.isinf(nr1)
    assert np.linalg.norm(x.download() - x0) <= 1e-10 and np.all(np.isnan(lam.download()))


def test_distances_one_two_agree_with_the_banded_operator(dev_ctx):
    """Distances (1, 2) are the banded operator of bandwidth 2 on the same data: equal count, x and lambda to 1e-12 (other kernels: not bits)."""
    ctx = dev_ctx
    n, m = 2049, 33
    a = 4.0 * synth.hash_vector(3, n) + 12.0                         # (lambda_min = 2.9, not diagonally dominant: the negative-weight Gram pass runs too)
    dists = (1, 2)
    offs = _rand_offs(n, dists, 3.0)
    U, Uh = _basis(ctx, n, m, False)
    b = ctx.vector(n, synth.hash_vector(4, n))
    offm = _off_matrix(ctx, n, offs, dists)
    res = []
    for A in (L.BandedOperator(0.5, ctx.vector(n, a - 0.5), offm, 2), L.DiagonalsOperator(0.5, ctx.vector(n, a - 0.5), offm, dists)):
        x, lam = ctx.vector(n), ctx.vector(m)
        it, nr = L.projcg_(x, lam, A, U, b, ctx.vector(m, np.linspace(-1, 1, m)), tol=1e-12, work=L.ProjCGWork(ctx, n, m))
        res.append((it, nr, x.download(), lam.download()))
    dx = np.linalg.norm(res[0][2] - res[1][2]) / np.linalg.norm(res[0][2])
    dl = np.abs(res[0][3] - res[1][3]).max() / np.abs(res[0][3]).max()
    print(f"[diags (1, 2) against band 2] iterations {res[1][0]} ({res[0][0]}), x {dx:.1e}, lambda {dl:.1e}")
    assert res[0][0] > 3 and res[0][0] == res[1][0]
    assert dx <= 1e-12 and dl <= 1e-12


def _solve_stacked_c(ctx, A, P, b, n, m, tol, maxit=None):
    """lfpsqp_projcg_diags itself over a stacked basis (no fall-back): rc, iterations, nr, x, lambda."""
    x, lam = L.StackedVector(ctx, n), ctx.vector(n + m)
    work = L.ProjCGWork(ctx, 0, m, stacked_N=n)
    Av = L.StackedVector(ctx, n)
    it, nr = _capi.c_i64(), C.c_double()
    u_c, w_c = P._c(), work._c()
    rc = ctx.L.lfpsqp_projcg_diags(ctx.h, x.h, lam.h, A.a0, A.dg.h, A.off.h, len(A.dists), A._dist_c, Av.h, C.byref(u_c), b.h, None, float(tol),
                                   int(2 * n + m if maxit is None else maxit), 2 * n, 1, C.byref(w_c), C.byref(it), C.byref(nr))
    return rc, it.value, nr.value, x, lam


@pytest.mark.parametrize("shape,m,kind,factored", [((30, 50), 16, "lap", False), ((8, 256), 128, "lap", True), ((3, 2100), 33, "lap", False),
                                                   ((12, 13, 14), 33, "lap", True), ((40, 50), 16, "lap9", False), ((3, 700), 33, "rand", False)])
def test_stacked_diagonals_solver_follows_the_oracle(dev_ctx, shape, m, kind, factored):
    """Four-way bounds: lfpsqp_projcg_diags over a stacked basis against the oracle's projcg! with the augmented map blockdiag(T, diag(ay)).
    The oracle's counts for these grids (7 .. 40 iterations) and the exit margins are printed by the test."""
    ctx = dev_ctx
    n = int(np.prod(shape))
    P, P0, _, rank = _stacked_problem(ctx, n, m, factored)
    assert rank == m
    ax, offs, dists, _ = _case_operator(shape, kind)
    ay = 0.5 + synth.hash_vector(16, n) ** 2
    A = _operator(ctx, ax, offs, dists, ay=ay)
    Aref = _DiagsRef(ax, offs, dists, ay)
    bh = synth.hash_vector(4, 2 * n)
    tmp = np.zeros(n + m)
    R.mul_(tmp, R.adj(P0), bh)
    R.mul_(bh, P0, tmp, -1.0, 1.0)                                      # a right-hand side in the tangent space, like optimize's d
    b = L.StackedVector(ctx, n).upload2(bh)
    tol_c, i_base, up, down = _conditioned_tol(Aref, P0, bh, np.zeros(n + m), n + m)
    print(f"[stacked diags] {shape} m={m} {kind} factored={factored}: oracle {i_base} iterations at 1e-10, tol {tol_c:.3e}, margins {up:.2f} / {down:.2f}")
    assert up >= 1.1 and down >= 1.1
    for tol, maxit in ((tol_c, None), (1e-300, 5)):
        x0, l0 = np.zeros(2 * n), np.zeros(n + m)
        i0, nr0 = R.projcg_(x0, l0, Aref, P0, bh, np.zeros(n + m), tol=tol, maxit=maxit)
        rc, i1, nr1, x, lam = _solve_stacked_c(ctx, A, P, b, n, m, tol, maxit)
        assert rc == 0
        xd, ld = x.download2(), lam.download()
        dx_ = np.linalg.norm(xd - x0) / np.linalg.norm(x0)
        dl_ = np.abs(ld - l0).max() / np.abs(l0).max()
        print(f"[stacked diags]   maxit={maxit}: iterations {i1} (oracle {i0}), nr {nr1:.6e} ({nr0:.6e}), x {dx_:.1e}, lambda {dl_:.1e}")
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


def _grid_pen(shape, kappa):
    def pen(v):                                                         # kappa L v from np.diff along each axis (zero flux across the border)
        V = v.reshape(shape)
        out = np.zeros(shape)
        for ax in range(len(shape)):
            pad = [(0, 0)] * len(shape)
            pad[ax] = (1, 1)
            out -= kappa * np.diff(np.pad(np.diff(V, axis=ax), pad), axis=ax)
        return out.ravel()
    return pen


@pytest.mark.parametrize("dim,cons", [(2, "eq"), (3, "eq"), (2, "box"), (3, "box"), (2, "ballbox"), (3, "ballbox")])
def test_grid_objective_follows_the_oracle(dev_ctx, dim, cons):
    """GridSeparableLinear: f = sum phi(x_i) + kappa/2 sum_{grid edges} (x_i - x_j)^2 through `optimize`.  Every truncated-Newton solve runs a
    DiagonalsOperator from the tangent step's state on lfpsqp_projcg_diags, and the trajectory is the oracle's with hess_lag_vec! built from
    np.diff along each axis.  Under bounds the oracle is run a second time from one ulp away, as in tests/test_tridiag_bounds.py."""
    ctx = dev_ctx
    emu = _is_emu(ctx)
    if emu:
        shape, m = ((16, 17), 4) if dim == 2 else ((6, 7, 8), 4)
    else:
        shape, m = ((60, 100), 16) if dim == 2 else ((15, 20, 20), 16)
    n = int(np.prod(shape))
    # Outer iterations compared on the GPU sizes: 8.  Measured on the ORACLE ALONE (box case, runs from x0 and from one ulp above and below it): its
    # own sensitivity stays at 1.0e-16 .. 2.3e-16 through outer iteration 8 (Newton systems of 3 .. 16 iterations) and then jumps by eight orders
    # of magnitude -- 1.6e-14 and 3.7e-08 at iterations 9 and 10 on the 60 x 100 grid (solves of 35 and 80 iterations), 2.7e-07 at iteration 9 on
    # the 15 x 20 x 20 one (a solve of 131) -- because bounds become active and one long projected-CG solve amplifies a last-bit difference.  From
    # there on a trajectory comparison measures the conditioning of that Newton system and whether its exit falls at iteration 79 or 80 (on the
    # MI355X the callback path took 79 where the oracle and the one-pass path took 80), not the kernels.
    maxiter = 4 if emu else 8
    kind, kappa = 1, 0.9
    a = 0.5 + synth.hash_vector(21, n) ** 2
    c = (1.3 if cons != "eq" else 0.3) * synth.hash_vector(22, n)
    phi, d1, d2 = _sep_host(kind, a, c)
    pen = _grid_pen(shape, kappa)
    v = synth.hash_vector(30, n)
    edges = sum(np.sum(np.diff(v.reshape(shape), axis=ax) ** 2) for ax in range(dim))
    assert abs(v @ pen(v) - kappa * edges) <= 1e-10 * abs(v @ pen(v))
    P0 = synth.BallBoxProblem(n, m)
    x0 = (0.9 * synth.hash_vector(2, n) + 0.05) if cons != "eq" else synth.hash_vector(2, n)
    f = lambda x: float(np.sum(phi(x[:n])) + 0.5 * kappa * sum(np.sum(np.diff(x[:n].reshape(shape), axis=ax) ** 2) for ax in range(dim)))

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
        P = L.GridSeparableLinear(ctx, shape, m, ctx.matrix(n + 1, m + 1).hash_fill(1, 0, n, 1.0, n, m), P0.eq.b, kind, a, c, kappa=kappa,
                                  R2=P0.R2, xl=P0.xl, xu=P0.xu)
    elif cons == "box":
        P = L.GridSeparableLinear(ctx, shape, m, ctx.matrix(n, m).hash_fill(1), P0.eq.b, kind, a, c, kappa=kappa, xl=P0.xl, xu=P0.xu)
    else:
        P = L.GridSeparableLinear(ctx, shape, m, ctx.matrix(n, m).hash_fill(1), P0.eq.b, kind, a, c, kappa=kappa)
    assert not hasattr(P, "offdiag") and not hasattr(P, "offdiags") and len(P.diagonals[0]) == dim and P.diagonals[1].m == dim
    import sys
    OPT = sys.modules["lfpsqp_jl_amd.optimize"]
    seen, rcs, orig = [], [], OPT.projcg_
    c_entry = ctx.L.lfpsqp_projcg_diags

    def spy(*args, **kw):
        seen.append((type(args[2]).__name__, bool(kw.get("start_given"))))
        return orig(*args, **kw)

    def c_spy(*args):
        rc = c_entry(*args)
        rcs.append(rc)
        return rc
    OPT.projcg_ = spy
    ctx.L.lfpsqp_projcg_diags = c_spy
    try:
        x, obj, lam, ti = P.optimize(x0, L.LFPSQPParams(disp=L.DisplayOption.off, **par), trace=tr)
    finally:
        OPT.projcg_ = orig
        ctx.L.lfpsqp_projcg_diags = c_entry
    assert seen and all(s == ("DiagonalsOperator", True) for s in seen)
    assert len(rcs) == len(seen) and all(rc == 0 for rc in rcs)
    assert ti.iter == tir.iter and ti.condition.name == tir.condition.name
    print(f"[grid {shape} {cons}] Newton-system iterations", [t.get('tn_iter') for t in tr0])
    assert any((t.get('tn_iter') or 0) > 3 for t in tr0)
    rtol = max(1e-10, 10.0 * max(sens))
    _note(f"grid objective {shape} ({cons}): the oracle's one-ulp sensitivity {max(sens):.1e}")
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


def _dist_array(*d):
    return (_capi.c_i64 * max(len(d), 1))(*d)


def test_diagonals_operator_is_refused_where_the_one_pass_form_does_not_exist(dev_ctx):
    """K outside 1 .. 4, distances that are not strictly increasing, below 1 or not below the row count, a null distance array and a view as the
    couplings are argument errors; a matrix view as basis and two columns are LFPSQP_ERR_UNSUPPORTED, and projcg_ then solves on the callback
    path; c != 0 with a stacked basis is unsupported, RESUME / START_PROJECTED are argument errors."""
    ctx = dev_ctx
    shape = (18, 50)
    n = 900
    deg, offs, dists = _laplacian(shape, 0.9)
    a = deg + 0.05 + 0.5 * synth.hash_vector(3, n) ** 2
    Aref = _DiagsRef(a, offs, dists)
    bh = synth.hash_vector(4, n)
    b = ctx.vector(n, bh)
    dg = ctx.vector(n, a)
    off4 = _off_matrix(ctx, n, offs + [np.zeros(n - 60), np.zeros(n - 70), np.zeros(n - 80)], dists + (60, 70, 80))
    A = L.DiagonalsOperator(0.0, dg, off4, dists)
    bad = [(0, _dist_array(1)), (5, _dist_array(1, 50, 60, 70, 80)), (2, _dist_array(50, 1)), (2, _dist_array(50, 50)), (2, _dist_array(0, 50)),
           (2, _dist_array(-1, 50)), (2, _dist_array(1, n)), (1, _dist_array(n + 5)), (2, None)]
    for m, view in ((2, False), (8, True), (8, False), (1025, False)):
        Uh, _ = np.linalg.qr(synth.hash_matrix(1, n, min(m, 8)))
        if m > 8:
            Uh = np.concatenate([Uh, np.zeros((n, m - 8))], axis=1)      # (refused for its width before any arithmetic)
        Uh = np.asfortranarray(Uh)
        Zd = ctx.matrix(n, m, Uh)
        U = L.DeviceBasis(Zd.view(ctx.vector(n, np.ones(n))) if view else Zd)
        x, lam, Av = ctx.vector(n), ctx.vector(m), ctx.vector(n)
        work = L.ProjCGWork(ctx, n, m)
        it, nr = _capi.c_i64(), C.c_double()
        u_c, w_c = U._c(), work._c()

        def solve(K, dist, flags=1, offh=off4.h):
            return ctx.L.lfpsqp_projcg_diags(ctx.h, x.h, lam.h, 0.0, dg.h, offh, K, dist, Av.h, C.byref(u_c), b.h, None, 1e-10, 100, n, flags,
                                             C.byref(w_c), C.byref(it), C.byref(nr))
        for K, dist in bad:
            assert solve(K, dist) == -1, (K, None if dist is None else list(dist))
            assert ctx.L.lfpsqp_diags_mul(ctx.h, 0.0, dg.h, off4.h, K, dist, b.h, Av.h) == -1, (K, None if dist is None else list(dist))
        if not view and m == 8:
            assert solve(2, A._dist_c, flags=1 | L.projcg.RESUME) == -1
            assert solve(2, A._dist_c, flags=1 | L.projcg.START_PROJECTED) == -1
            assert solve(2, A._dist_c) == 0 and it.value > 3
            continue
        assert solve(2, A._dist_c) == -5
        if m > 8:
            continue
        tol, i_base, up, down = _conditioned_tol(Aref, Uh, bh, np.zeros(m), m)
        assert up >= 1.1 and down >= 1.1
        x0, l0 = np.zeros(n), np.zeros(m)
        i0, nr0 = R.projcg_(x0, l0, Aref, Uh, bh, np.zeros(m), tol=tol)
        x, lam = ctx.vector(n), ctx.vector(m)
        i1, nr1 = L.projcg_(x, lam, A, U, b, None, tol=tol, work=work)
        assert i1 == i0 and np.linalg.norm(x.download() - x0) <= 1e-10 * np.linalg.norm(x0)
    # a view as the couplings
    offv = off4.view(ctx.vector(n, np.ones(n)))
    Av = ctx.vector(n)
    assert ctx.L.lfpsqp_diags_mul(ctx.h, 0.0, dg.h, offv.h, 2, A._dist_c, b.h, Av.h) == -1
    # stacked basis with c != 0
    ns, ms = 600, 8
    P, P0, _, rank = _stacked_problem(ctx, ns, ms, False)
    degs, offss, distss = _laplacian((12, 50), 0.9)
    As = _operator(ctx, degs + 1.0, offss, distss, ay=np.ones(ns))
    xs, lams, Avs = L.StackedVector(ctx, ns), ctx.vector(ns + ms), L.StackedVector(ctx, ns)
    works = L.ProjCGWork(ctx, 0, ms, stacked_N=ns)
    bs = L.StackedVector(ctx, ns).upload2(synth.hash_vector(4, 2 * ns))
    it, nr = _capi.c_i64(), C.c_double()
    u_c, w_c = P._c(), works._c()
    cvec = ctx.vector(ns + ms, np.ones(ns + ms))
    rc = ctx.L.lfpsqp_projcg_diags(ctx.h, xs.h, lams.h, As.a0, As.dg.h, As.off.h, 2, As._dist_c, Avs.h, C.byref(u_c), bs.h, cvec.h, 1e-10, 100,
                                   2 * ns, 1, C.byref(w_c), C.byref(it), C.byref(nr))
    assert rc == -5


def test_diagonals_operator_refuses_row_shards(emu_lib):
    """A communicator (the row-shard case): the one-pass solve and the product answer LFPSQP_ERR_UNSUPPORTED; projcg_ raises."""
    ctx = L.Context(0, emu_lib)
    try:
        ctx.comm_init_callback(0, 1, lambda ptr, count, op, stream: 0)
        n, m = 700, 8
        deg, offs, dists = _laplacian((14, 50), 0.9)
        A = _operator(ctx, deg + 1.0, offs, dists)
        Uh, _ = np.linalg.qr(synth.hash_matrix(1, n, m))
        U = L.DeviceBasis(ctx.matrix(n, m, np.asfortranarray(Uh)))
        b, x, lam, Av = ctx.vector(n, synth.hash_vector(4, n)), ctx.vector(n), ctx.vector(m), ctx.vector(n)
        work = L.ProjCGWork(ctx, n, m)
        it, nr = _capi.c_i64(), C.c_double()
        u_c, w_c = U._c(), work._c()
        rc = ctx.L.lfpsqp_projcg_diags(ctx.h, x.h, lam.h, 0.0, A.dg.h, A.off.h, 2, A._dist_c, Av.h, C.byref(u_c), b.h, None, 1e-10, 100, n, 1,
                                       C.byref(w_c), C.byref(it), C.byref(nr))
        assert rc == -5
        assert ctx.L.lfpsqp_diags_mul(ctx.h, 0.0, A.dg.h, A.off.h, 2, A._dist_c, b.h, Av.h) == -5
        with pytest.raises(L.LfpsqpError):
            L.projcg_(x, lam, A, U, b, None, tol=1e-10, work=work)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_diagonals_projcg_at_protocol_size(gpu_lib):
    """(1e6, 128), the 1000 x 1000 grid, kappa L + a: equal counts and iterates within 1e-10 of the oracle."""
    ctx = L.Context(0, gpu_lib)
    try:
        shape, m = (1000, 1000), 128
        n = 1_000_000
        deg, off, dists = L.grid_laplacian(shape, 0.9)
        offs = [off[:n - s, k].copy() for k, s in enumerate(dists)]
        a = deg + 0.05 + 0.5 * synth.hash_vector(3, n) ** 2
        U, Uh = _basis(ctx, n, m, False)
        bh = synth.hash_vector(4, n)
        Aref = _DiagsRef(a, offs, dists)
        tol, i_base, up, down = _conditioned_tol(Aref, Uh, bh, np.zeros(m), m)
        print(f"[diags 1e6] oracle {i_base} iterations at 1e-10, tol {tol:.3e}, margins {up:.2f} / {down:.2f}")
        assert up >= 1.1 and down >= 1.1
        x0, l0 = np.zeros(n), np.zeros(m)
        i0, nr0 = R.projcg_(x0, l0, Aref, Uh, bh, np.zeros(m), tol=tol)
        x, lam = ctx.vector(n), ctx.vector(m)
        i1, nr1 = L.projcg_(x, lam, _operator(ctx, a, offs, dists), U, ctx.vector(n, bh), None, tol=tol, work=L.ProjCGWork(ctx, n, m))
        dx = np.linalg.norm(x.download() - x0) / np.linalg.norm(x0)
        dl = np.abs(lam.download() - l0).max()
        print(f"[diags 1e6] iterations {i1} (oracle {i0}), x {dx:.1e}, lambda {dl:.1e}")
        assert i1 == i0 and i1 > 3 and dx <= 1e-10 and dl <= 1e-10
    finally:
        ctx.close()
