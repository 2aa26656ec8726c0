"""Non-quadratic edge potentials on a graph, and sparse Hessian values refreshed on the device: lfpsqp_sphess_like, lfpsqp_sphess_edge_eval and
the host layers above them (SparseHessian.like / .edge_eval, GraphPotentialLinear).

With t = x_i - x_j per undirected edge:  f = scale sum_e w_e psi(t),  grad_i += scale sum_j w_ij psi'(x_i - x_j),  diag_i += scale sum_j w_ij
psi''(x_i - x_j),  and the value of H at every stored edge, in both ELL forms, = -(scale w_e) psi''(t).  There is no value download in the ABI: H is
observed through lfpsqp_sphess_mul (unit vectors on the small graph, one indicator vector per colour class of a distance-2 colouring elsewhere --
both read entries back exactly).  Graphs and the reference operator come from tests/test_projcg_sparse.py.

ROUNDING COUNTS, from the expressions of csrc/sphess_edge.hip as written, against a reference that takes t = x_i - x_j EXACTLY from the fp64 x
(u = 2^-53; a count k stands for the factor gamma_k):
    t = fl(x_i - x_j): 1.   q = fl(t t): 3.
    kind 1:  psi = fma(q/4, q, q/2): 7 (q^2 carries 6, the sum of two positive parts at most that, + 1).  psi' = fma(q, t, t): 5 (t^3 carries
             4, + 1).  psi'' = fma(3, q, 1): 4.
    kind 2:  rd2 = 1 / fl(delta delta) on the host: 2.  a = fma(q, rd2, 1): 6 (q rd2 carries 5 and is at most a, + 1).  s = sqrt(a): 4 (half of
             6, + 1).  psi = q / (s + 1): 9 (s + 1 carries 5; 3 + 5 + 1).  psi' = t / s: 6.  psi'' = 1 / (a s): 12 (6 + 4 + 1, + 1).
    a row sum (grad, diag): every term passes through at most Kr additions of the fma chain (the products with w are inside the fmas), and one
             more rounding in  fma(scale, sum, 0):  c = count(psi' or psi'') + 1, i.e.  c_grad = 6 / 7  and  c_diag = 5 / 13  for kinds 1 / 2,
             and the bound is gamma_{Kr + c} sum_k |term_k|.
    an entry of H:  fl(scale w) and the product with psi'':  c' = count(psi'') + 2 = 6 / 14.
    f: a term carries count(psi) = 7 / 9 and then passes, in whatever order lanes, waves, blocks and the second stage take them, through at most
             (n Kr - 1) additions, + 1 for the zero-initialised accumulators, + 1 for the product with scale (halving is exact):
             gamma_{n Kr + count(psi) + 1} sum |terms|  (the arbitrary-order bound of tests/test_primitives_exact.py (c)).
No count exceeds 16.  The observed maxima are printed next to each bound."""
import ctypes as C
import sys

import numpy as np
import pytest

import lfpsqp_jl_amd as L
from oracle import lfpsqp_ref as R
from oracle import synth

from .helpers import POISON, bits, gamma
from .test_capi_retractions import _compare_traces, _note, _sep_host
from .test_projcg_diags import _basis, _conditioned_tol
from .test_projcg_sparse import KAPPA, _graph, _GraphRef

C_PSI = {1: 7, 2: 9}
C_GRAD = {1: 6, 2: 7}
C_DIAG = {1: 5, 2: 13}
C_H = {1: 6, 2: 14}
DELTA = 0.5


def _g(k):
    return float(gamma(k))


# ---- observing H ---------------------------------------------------------------------------------------------------------------------------
def _mul(ctx, S, vh, a0=0.0, dg=None):
    out = ctx.vector(len(vh))
    L.SparseOperator(a0, dg, S).mul_(out, ctx.vector(len(vh), vh))
    return out.download()


def _dense(ctx, S, n):
    """H column by column: S e_j, exact (one product and additions of zeros per entry)."""
    D = np.empty((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        D[:, j] = _mul(ctx, S, e)
        e[j] = 0.0
    return D


_COLOURS = {}


def _colours(name):
    """A greedy distance-2 colouring: no row has two neighbours of one colour, so S 1_{colour} holds S_ij at row i for its only neighbour j of that
    colour -- every entry of both triangles read back exactly with one product per colour."""
    if name not in _COLOURS:
        n, ei, ej = _graph(name)
        nb = [[] for _ in range(n)]
        for a, b in zip(ei.tolist(), ej.tolist()):
            nb[a].append(b)
            nb[b].append(a)
        col = np.full(n, -1)
        for v in range(n):
            used = {col[u] for r in nb[v] for u in nb[r] if u != v}
            k = 0
            while k in used:
                k += 1
            col[v] = k
        _COLOURS[name] = col
    return _COLOURS[name]


def _entries(ctx, S, name):
    """(S[i_e, j_e], S[j_e, i_e]) per edge of the graph."""
    n, ei, ej = _graph(name)
    col = _colours(name)
    up, lo = np.empty(len(ei)), np.empty(len(ei))
    for k in range(col.max() + 1):
        out = _mul(ctx, S, (col == k).astype(np.float64))
        sel = col[ej] == k
        up[sel] = out[ei[sel]]
        sel = col[ei] == k
        lo[sel] = out[ej[sel]]
    return up, lo


# ---- references ------------------------------------------------------------------------------------------------------------------------------
def _int_case(name, seed):
    """Integer weights 1 .. 4 and integer x in [-6, 6]: |t| <= 12, w t^4 <= 82944, every sum far below 2^53."""
    n, ei, ej = _graph(name)
    rng = np.random.default_rng(seed)
    return n, ei, ej, rng.integers(1, 5, len(ei)), rng.integers(-6, 7, n)


def _int_reference(n, ei, ej, w, x, kind):
    """(4 f, grad, diag, h) in int64: kind 0: psi = t^2/2, kind 1: t^2/2 + t^4/4."""
    t = x[ei] - x[ej]
    psi4 = 2 * t * t + (t ** 4 if kind else 0)
    p1 = t + (t ** 3 if kind else 0)
    p2 = 1 + (3 * t * t if kind else 0)
    bc = lambda idx, val: np.bincount(idx, val.astype(np.float64), n).astype(np.int64)       # (sums of integers below 2^53: exact)
    return int(np.sum(w * psi4)), bc(ei, w * p1) - bc(ej, w * p1), bc(ei, w * p2) + bc(ej, w * p2), -(w * p2)


def _psi_np(kind, t, delta):
    """psi, psi', psi'' in numpy float64 with the kernel's expressions (the oracle side of GraphPotentialLinear and of the large case)."""
    q = t * t
    if kind == 0:
        return 0.5 * q, t, np.ones_like(t)
    if kind == 1:
        return 0.25 * q * q + 0.5 * q, q * t + t, 3.0 * q + 1.0
    a = q * (1.0 / (delta * delta)) + 1.0
    s = np.sqrt(a)
    return q / (s + 1.0), t / s, 1.0 / (a * s)


def _real_case(name):
    n, ei, ej = _graph(name)
    return n, ei, ej, 0.5 + synth.hash_vector(51, len(ei)) ** 2, 2.4 * synth.hash_vector(52, n) - 1.2


_MP = {}


def _mp_reference(name, kind, scale):
    """The definitions in mpmath at 60 digits, t exactly from the fp64 x: per edge psi, psi', psi'' as mpf; once per case, shared by both devices."""
    key = (name, kind)
    if key not in _MP:
        import mpmath
        n, ei, ej, w, x = _real_case(name)
        with mpmath.workdps(60):
            mp = mpmath.mpf
            d = mp(DELTA)
            rows = []
            for a, b, we in zip(ei.tolist(), ej.tolist(), w.tolist()):
                t = mp(float(x[a])) - mp(float(x[b]))
                if kind == 1:
                    p0, p1, p2 = t * t / 2 + t ** 4 / 4, t + t ** 3, 1 + 3 * t * t
                else:
                    r = mpmath.sqrt(1 + (t / d) ** 2)
                    p0, p1, p2 = d * d * (r - 1), t / r, 1 / ((1 + (t / d) ** 2) * r)
                sw = mp(scale) * mp(we)
                rows.append((sw * p0, sw * p1, sw * p2))
            _MP[key] = rows
    return _MP[key]


# ---- 1. exact, integer data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [None, 2])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", ["pc567", "hub32", "mesh45"])
def test_integer_data_is_exact(dev_ctx, monkeypatch, name, kind, blocks):
    """f, grad, diag and every entry of H `==` the int64 reference; once more with LFPSQP_VEC_BLOCKS = 2, where a block walks several tiles (mesh45:
    five tiles in two blocks) before the second reduction stage."""
    if blocks is not None:
        monkeypatch.setenv("LFPSQP_VEC_BLOCKS", str(blocks))
    ctx = L.Context(0, dev_ctx.L) if blocks is not None else dev_ctx
    try:
        n, ei, ej, w, xh = _int_case(name, 7 + kind)
        f4, gr, dr, hr = _int_reference(n, ei, ej, w, xh, kind)
        W = L.SparseHessian(ctx, n, ei, ej, w.astype(np.float64))
        H = W.like()
        x, g, d = ctx.vector(n, xh.astype(np.float64)), ctx.vector(n), ctx.vector(n)
        f = W.edge_eval(kind, 1.0, 1.0, x, g, d, H)
        assert f == f4 / 4.0 and W.edge_eval(kind, 1.0, 1.0, x) == f4 / 4.0            # (the full call and the kernel that only reads)
        assert np.array_equal(g.download(), gr) and np.array_equal(d.download(), dr)
        if name == "pc567":
            D = np.zeros((n, n))
            D[ei, ej] = D[ej, ei] = hr
            assert np.array_equal(_dense(ctx, H, n), D)
        else:
            up, lo = _entries(ctx, H, name)
            assert np.array_equal(up, hr) and np.array_equal(lo, hr)
        vh = np.random.default_rng(3).integers(-9, 10, n).astype(np.float64)
        assert np.array_equal(_mul(ctx, H, vh), _GraphRef(n, ei, ej, hr.astype(np.float64), np.zeros(n))._op(vh))
    finally:
        if blocks is not None:
            ctx.close()


# ---- 2. real data against mpmath -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("name", ["pc567", "hub32"])
def test_real_data_within_the_counted_bounds(dev_ctx, name, kind):
    """Kinds 1 and 2 (delta = 0.5), scale = 0.9, w in [0.5, 1.5], x in [-1.2, 1.2], against the definitions at 60 digits; the counts are those of the
    module docstring: per row gamma_{Kr + c} sum_k |term_k| with c = 6 / 7 (grad) and 5 / 13 (diag), f within gamma_{n Kr + 8 / 10} sum |terms|,
    the entries of H within gamma_{6 / 14} relative."""
    ctx = dev_ctx
    n, ei, ej, w, xh = _real_case(name)
    ref = _mp_reference(name, kind, KAPPA)
    W = L.SparseHessian(ctx, n, ei, ej, w)
    H = W.like()
    kr = W.row_width
    x, g, d = ctx.vector(n, xh), ctx.vector(n), ctx.vector(n)
    f = W.edge_eval(kind, DELTA, KAPPA, x, g, d, H)
    f_only = W.edge_eval(kind, DELTA, KAPPA, x)
    gd, dd = g.download(), d.download()
    import mpmath
    with mpmath.workdps(60):
        mp = mpmath.mpf
        zero = mp(0)
        gx, ga, dx = [zero] * n, [zero] * n, [zero] * n
        for (p0, p1, p2), a, b in zip(ref, ei.tolist(), ej.tolist()):
            gx[a] += p1
            gx[b] -= p1
            ga[a] += abs(p1)
            ga[b] += abs(p1)
            dx[a] += p2
            dx[b] += p2
        fx = mpmath.fsum(r[0] for r in ref)                                  # (positive terms: sum |terms| = f, each edge once)
        eg = max(float(abs(mp(float(gd[i])) - gx[i]) / ga[i]) for i in range(n) if ga[i] > 0)
        ed = max(float(abs(mp(float(dd[i])) - dx[i]) / dx[i]) for i in range(n) if dx[i] > 0)
        ef = max(float(abs(mp(v) - fx) / fx) for v in (f, f_only))
        up, lo = (_dense(ctx, H, n)[idx] for idx in ((ei, ej), (ej, ei))) if name == "pc567" else _entries(ctx, H, name)
        eh = max(float(abs(mp(float(v)) + r[2]) / r[2]) for arr in (up, lo) for v, r in zip(arr.tolist(), ref))
    print(f"[edge eval] {name} kind {kind} Kr {kr}: grad {eg:.2e} (bound {_g(kr + C_GRAD[kind]):.2e}), diag {ed:.2e} ({_g(kr + C_DIAG[kind]):.2e}), "
          f"f {ef:.2e} ({_g(n * kr + C_PSI[kind] + 1):.2e}), H {eh:.2e} ({_g(C_H[kind]):.2e})")
    assert eg <= _g(kr + C_GRAD[kind])
    assert ed <= _g(kr + C_DIAG[kind])
    assert ef <= _g(n * kr + C_PSI[kind] + 1)
    assert eh <= _g(C_H[kind])
    assert all(gd[i] == 0.0 for i in range(n) if ga[i] == 0)


# ---- 3. symmetry and form agreement ------------------------------------------------------------------------------------------------------------
def test_refreshed_handle_is_symmetric_and_solves_like_the_oracle(dev_ctx):
    """After a kind-2 refresh on pc567 the columns of H form a matrix exactly equal to its transpose, and lfpsqp_projcg_sparse on it (its set-up reads
    the EDGE form, its products the row form) runs the oracle's count with iterates within 1e-10 of projcg! with the np.bincount operator of the
    values read back; the exit-condition rule and its 1.1 margins are those of tests/test_projcg_sparse.py."""
    ctx = dev_ctx
    m = 6
    n, ei, ej, w, xh = _real_case("pc567")
    W = L.SparseHessian(ctx, n, ei, ej, w)
    H = W.like()
    base = 0.05 + 0.5 * synth.hash_vector(3, n) ** 2
    dg = ctx.vector(n, base)
    W.edge_eval(2, DELTA, KAPPA, ctx.vector(n, xh), None, dg, H, want_f=False)
    D = _dense(ctx, H, n)
    assert np.array_equal(D, D.T)
    v = D[ei, ej]
    assert np.all(v < 0) and np.count_nonzero(D) == 2 * len(ei)
    p2 = _psi_np(2, xh[ei] - xh[ej], DELTA)[2]
    assert v.max() / v.min() < 0.2 and np.abs(v + KAPPA * w * p2).max() <= 1e-14       # (the values move by more than a factor 5 over the edges)
    Aref = _GraphRef(n, ei, ej, v, dg.download())
    U, Uh = _basis(ctx, n, m, False)
    bh = synth.hash_vector(4, n)
    tol, i_base, up, down = _conditioned_tol(Aref, Uh, bh, np.zeros(m), m)
    print(f"[edge eval] refreshed pc567: oracle {i_base} iterations at 1e-10, tol {tol:.3e}, margins {up:.2f} / {down:.2f}")
    assert up >= 1.1 and down >= 1.1
    x0, l0 = np.zeros(n), np.zeros(m)
    i0, nr0 = R.projcg_(x0, l0, Aref, Uh, bh, np.zeros(m), tol=tol)
    x, lam = ctx.vector(n), ctx.vector(m)
    i1, nr1 = L.projcg_(x, lam, L.SparseOperator(0.0, dg, H), U, ctx.vector(n, bh), None, tol=tol, work=L.ProjCGWork(ctx, n, m))
    dx = np.linalg.norm(x.download() - x0) / np.linalg.norm(x0)
    dl = np.abs(lam.download() - l0).max()
    print(f"[edge eval]   iterations {i1} (oracle {i0}), nr {nr1:.6e} ({nr0:.6e}), x {dx:.1e}, lambda {dl:.1e}")
    assert i1 == i0 == i_base and i1 > 3 and nr1 == pytest.approx(nr0, rel=1e-5)
    assert dx <= 1e-10 and dl <= 1e-10


# ---- 4. kind 0 is the constant class -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pc567", "hub32", "mesh45"])
def test_kind_0_gives_the_bits_of_a_handle_created_from_the_values(dev_ctx, name):
    ctx = dev_ctx
    n, ei, ej, w, xh = _real_case(name)
    W = L.SparseHessian(ctx, n, ei, ej, w)
    H = W.like()
    W.edge_eval(0, 0.0, KAPPA, ctx.vector(n, xh), out=H, want_f=False)
    S = L.SparseHessian(ctx, n, ei, ej, -(KAPPA * w))               # what GraphSeparableLinear builds on the host
    vh = synth.hash_vector(7, n)
    dg = ctx.vector(n, 1.0 + synth.hash_vector(3, n))
    got, want = _mul(ctx, H, vh, 0.25, dg), _mul(ctx, S, vh, 0.25, dg)
    assert np.array_equal(bits(got), bits(want)) and np.any(got != (1.25 + synth.hash_vector(3, n)) * vh)


# ---- 5. accumulation and ranges ----------------------------------------------------------------------------------------------------------------
def test_outputs_accumulate_and_leave_everything_else_alone(dev_ctx):
    """grad and diag are added to; entries >= W.n (a slack row, the gap and the y half of a stacked vector) keep their bits; a stacked x is read on
    its x half; every output may be NULL; the value-only call leaves H's bits; W is never modified."""
    ctx = dev_ctx
    n, ei, ej, w, xh = _int_case("mesh45", 11)
    f4, gr, dr, hr = _int_reference(n, ei, ej, w, xh, 1)
    W = L.SparseHessian(ctx, n, ei, ej, w.astype(np.float64))
    H = W.like()
    vh = np.random.default_rng(4).integers(-9, 10, n).astype(np.float64)
    w_before, h_before = _mul(ctx, W, vh), _mul(ctx, H, vh)
    assert np.array_equal(bits(w_before), bits(h_before))           # (like: initialised to W's values)
    x = L.StackedVector(ctx, n).upload2(np.concatenate([xh, np.full(n, 1e3)]).astype(np.float64))
    g0 = np.random.default_rng(5).integers(-50, 51, n + 1).astype(np.float64)
    g0[n] = POISON                                                  # the slack row of a gradient of n + 1 entries
    g = ctx.vector(n + 1, g0)
    d = L.StackedVector(ctx, n).upload2(np.concatenate([g0[:n], np.full(n, POISON)]))
    d_all = d.download()
    assert W.edge_eval(1, 1.0, 1.0, x) == f4 / 4.0                  # value only: nothing written
    assert np.array_equal(bits(_mul(ctx, H, vh)), bits(h_before))
    assert np.array_equal(bits(g.download()), bits(g0)) and np.array_equal(bits(d.download()), bits(d_all))
    assert W.edge_eval(1, 1.0, 1.0, x, grad=g, want_f=False) is None
    assert np.array_equal(g.download()[:n], g0[:n] + gr) and bits(g.download()[n:])[0] == bits([POISON])[0]
    assert np.array_equal(bits(d.download()), bits(d_all)) and np.array_equal(bits(_mul(ctx, H, vh)), bits(h_before))
    assert W.edge_eval(1, 1.0, 1.0, x, diag=d) == f4 / 4.0
    got = d.download()
    assert np.array_equal(got[:n], g0[:n] + dr) and np.array_equal(bits(got[n:]), bits(d_all[n:]))
    assert np.array_equal(bits(_mul(ctx, H, vh)), bits(h_before))
    W.edge_eval(1, 1.0, 1.0, x, grad=g, diag=d, out=H, want_f=False)                      # a second time: added again
    assert np.array_equal(g.download()[:n], g0[:n] + 2 * gr) and np.array_equal(d.download()[:n], g0[:n] + 2 * dr)
    assert np.array_equal(_mul(ctx, H, vh), _GraphRef(n, ei, ej, hr.astype(np.float64), np.zeros(n))._op(vh))
    assert W.edge_eval(1, 1.0, 1.0, x, out=H, want_f=False) is None
    ctx.check(ctx.L.lfpsqp_sphess_edge_eval(ctx.h, W.h, 1, 1.0, 1.0, x.h, None, None, None, None))     # nothing asked for
    assert np.array_equal(bits(_mul(ctx, W, vh)), bits(w_before))


# ---- 6. like and lifetime ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["W", "H"])
def test_like_shares_the_pattern_and_either_handle_may_go_first(dev_ctx, first):
    ctx = dev_ctx
    n, ei, ej, w, xh = _int_case("hub32", 13)
    f4, gr, dr, hr = _int_reference(n, ei, ej, w, xh, 1)
    W = L.SparseHessian(ctx, n, ei, ej, w.astype(np.float64))
    H = W.like()
    H2 = H.like()                                                   # (a handle on the pattern of a handle on the pattern)
    info = lambda S: (S.n, S.nedges, S.row_width, S.edge_width)
    assert info(W) == info(H) == info(H2) == (n, len(ei), 32, W.edge_width)
    x = ctx.vector(n, xh.astype(np.float64))
    vh = np.random.default_rng(6).integers(-9, 10, n).astype(np.float64)
    want_h = _GraphRef(n, ei, ej, hr.astype(np.float64), np.zeros(n))._op(vh)
    want_w = _GraphRef(n, ei, ej, w.astype(np.float64), np.zeros(n))._op(vh)
    W.edge_eval(1, 1.0, 1.0, x, out=H, want_f=False)
    if first == "W":
        W.close()
        assert np.array_equal(_mul(ctx, H, vh), want_h) and np.array_equal(_mul(ctx, H2, vh), want_w)
        H2.edge_eval(1, 1.0, 1.0, x, out=H, want_f=False)           # the pattern is alive: evaluate from the weights H2 kept
        assert np.array_equal(_mul(ctx, H, vh), want_h)
        H.close()
        assert np.array_equal(_mul(ctx, H2, vh), want_w)
        H2.close()
    else:
        H.close()
        H2.close()
        assert np.array_equal(_mul(ctx, W, vh), want_w)
        g = ctx.vector(n)
        assert W.edge_eval(1, 1.0, 1.0, x, grad=g) == f4 / 4.0 and np.array_equal(g.download(), gr)
        W.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------------
def _refusal_setup(ctx):
    n, ei, ej, w, xh = _real_case("pc567")
    W = L.SparseHessian(ctx, n, ei, ej, w)
    return n, W, W.like(), L.SparseHessian(ctx, n, ei, ej, w), ctx.vector(n, xh), ctx.vector(n), ctx.vector(n)


def test_edge_eval_refuses_bad_arguments(dev_ctx):
    ctx = dev_ctx
    n, W, H, other, x, g, d = _refusal_setup(ctx)
    f = C.c_double()

    def call(kind=2, delta=DELTA, scale=1.0, xx=x, gg=g, dd=d, hh=H, ww=W):
        h = lambda o: None if o is None else o.h
        return ctx.L.lfpsqp_sphess_edge_eval(ctx.h, h(ww), kind, delta, scale, h(xx), C.byref(f), h(gg), h(dd), h(hh))
    assert call() == 0
    assert call(kind=-1) == -1 and call(kind=3) == -1
    for bad in (0.0, -0.5, np.nan, np.inf):
        assert call(delta=bad) == -1
        assert call(kind=1, delta=bad) == 0                         # (delta belongs to kind 2 alone)
    for bad in (np.nan, np.inf, -np.inf):
        assert call(scale=bad) == -1
    short = ctx.vector(n - 1)
    assert call(xx=short) == -1 and call(gg=short) == -1 and call(dd=short) == -1
    assert call(gg=x) == -1 and call(dd=x) == -1 and call(gg=g, dd=g) == -1              # aliasing
    assert call(hh=other) == -1                                     # the same graph, another pattern object
    assert call(hh=W) == -1                                         # H == W: the weights would be lost
    assert call(ww=None) == -1 and call(xx=None) == -1
    out = C.c_void_p()
    assert ctx.L.lfpsqp_sphess_like(ctx.h, None, C.byref(out)) == -1 and ctx.L.lfpsqp_sphess_like(ctx.h, W.h, None) == -1
    assert call(xx=L.StackedVector(ctx, n), gg=None, dd=None) == 0  # a longer x is fine
    assert call(hh=None) == 0 and call() == 0


def test_edge_eval_refuses_row_shards_and_foreign_handles(emu_lib):
    ctx = L.Context(0, emu_lib)
    ctx2 = L.Context(0, emu_lib)
    try:
        n, W, H, other, x, g, d = _refusal_setup(ctx)
        H2 = L.SparseHessian(ctx2, n, *_graph("pc567")[1:], 1.0)
        with pytest.raises(ValueError):
            W.edge_eval(2, DELTA, 1.0, x, out=H2)
        H2.close()
        assert W.edge_eval(2, DELTA, 1.0, x, g, d, H) > 0
        ctx.comm_init_callback(0, 1, lambda ptr, count, op, stream: 0)
        f = C.c_double()
        assert ctx.L.lfpsqp_sphess_edge_eval(ctx.h, W.h, 2, DELTA, 1.0, x.h, C.byref(f), g.h, d.h, H.h) == -5
        assert ctx.L.lfpsqp_sphess_edge_eval(ctx.h, W.h, 2, DELTA, 1.0, x.h, C.byref(f), None, None, None) == -5
        with pytest.raises(L.LfpsqpError):
            W.edge_eval(2, DELTA, 1.0, x)
    finally:
        ctx2.close()
        ctx.close()


# ---- 8. GraphPotentialLinear through optimize --------------------------------------------------------------------------------------------------
_ORACLE_RUNS = {}
_PAR = dict(do_project_retract=False, maxiter=8, tn_kappa=1e-6)


def _oracle_runs(edge_kind, delta, n, ei, ej, m, kind, a, c, P0, x0):
    """The oracle's run and its run from one ulp away; once per case, shared by the emulator and GPU runs, read-only."""
    key = (edge_kind, delta)
    if key not in _ORACLE_RUNS:
        phi, d1, d2 = _sep_host(kind, a, c)
        psi = lambda x: _psi_np(edge_kind, x[ei] - x[ej], delta)
        spread = []

        def f(x):
            return float(np.sum(phi(x[:n])) + KAPPA * np.sum(psi(x)[0]))

        def grad_(g, x):
            p1 = psi(x)[1]
            g[:n] = d1(x[:n]) + KAPPA * (np.bincount(ei, p1, n) - np.bincount(ej, p1, n))

        def hlv_(dest, src, x, lam):
            p2 = KAPPA * psi(x)[2]
            spread.append((np.abs(x[ei] - x[ej]).max(), p2.min() / KAPPA))
            dest[:] = (d2(x) + 2.0 * lam[m]) * src + _GraphRef(n, ei, ej, -p2, np.bincount(ei, p2, n) + np.bincount(ej, p2, n))._op(src)

        def oracle(xs, trace):
            p = R.LFPSQPParams(disp=R.DisplayOption.off, **_PAR)
            dv0 = P0.derivatives()
            return R.optimize(f, P0.c_, P0.d_, xs, P0.xl, P0.xu, m, 1, p,
                              derivatives=R.Derivatives(grad_=grad_, hess_lag_vec_=hlv_, jac_c_=dv0.jac_c_, jac_d_=dv0.jac_d_), trace=trace)
        tr0, tr1 = [], []
        xr, objr, lamr, tir = oracle(x0, tr0)
        oracle(np.nextafter(x0, np.inf), tr1)
        sens = [np.linalg.norm(p['x'] - q['x']) / np.linalg.norm(q['x']) for p, q in zip(tr1, tr0)] + [np.inf] * (len(tr0) - len(tr1))
        _ORACLE_RUNS[key] = (tr0, xr, objr, tir, sens, max(s[0] for s in spread), min(s[1] for s in spread))
    return _ORACLE_RUNS[key]


@pytest.mark.parametrize("edge_kind,delta", [(2, 0.5), (1, 1.0), (2, 0.1)])
def test_graph_potential_objective_follows_the_oracle(dev_ctx, edge_kind, delta):
    """GraphPotentialLinear on the 26-neighbour periodic grid with ball and box through `optimize`: every truncated-Newton solve runs a SparseOperator
    from the tangent step's state on lfpsqp_projcg_sparse, on values refreshed at the current x, and the trajectory is the oracle's with
    hess_lag_vec! a matrix-free map over the edge list whose weights are psi''(x_i - x_j).  Structure, spies and the one-ulp sensitivity rule are
    those of tests/test_projcg_sparse.py::test_graph_objective_follows_the_oracle.  On the oracle alone: sensitivity 1.1e-16 (kind 2, delta 0.5),
    1.2e-16 (kind 1), 1.3e-16 (delta 0.1); 2-5 Newton-system iterations per outer iteration; |x_i - x_j| reaches 2.7 (delta 0.5), where psi''
    spans 1 down to 0.006: stale values cannot pass."""
    ctx = dev_ctx
    n, ei, ej = _graph("pc567")
    m, kind = 4, 1
    a = 0.5 + synth.hash_vector(21, n) ** 2
    c = 1.3 * synth.hash_vector(22, n)
    P0 = synth.BallBoxProblem(n, m)
    x0 = 0.9 * synth.hash_vector(2, n) + 0.05
    par = _PAR
    tr = []
    tr0, xr, objr, tir, sens, tmax, p2min = _oracle_runs(edge_kind, delta, n, ei, ej, m, kind, a, c, P0, x0)
    print(f"[graph potential pc567 kind {edge_kind} delta {delta}] largest |x_i - x_j| {tmax:.2f}, smallest psi'' {p2min:.4f}")
    P = L.GraphPotentialLinear(ctx, n, m, ctx.matrix(n + 1, m + 1).hash_fill(1, 0, n, 1.0, n, m), P0.eq.b, kind, a, c, edges=(ei, ej, 1.0),
                               kappa=KAPPA, edge_kind=edge_kind, delta=delta, R2=P0.R2, xl=P0.xl, xu=P0.xu)
    S = P.sparse_hessian
    assert (S.n, S.nedges, S.row_width) == (n + 1, len(ei), 26)    # (the slack row has no couplings)
    OPT = sys.modules["lfpsqp_jl_amd.optimize"]
    seen, rcs, orig = [], [], OPT.projcg_
    c_entry = ctx.L.lfpsqp_projcg_sparse

    def spy(*args, **kw):
        seen.append((type(args[2]).__name__, bool(kw.get("start_given")), args[2].S is S))
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
    assert seen and all(s == ("SparseOperator", True, True) for s in seen)
    assert len(rcs) == len(seen) and all(rc == 0 for rc in rcs)
    assert ti.iter == tir.iter and ti.condition.name == tir.condition.name
    print(f"[graph potential pc567 kind {edge_kind} delta {delta}] Newton-system iterations", [t.get('tn_iter') for t in tr0])
    assert any((t.get('tn_iter') or 0) >= 2 for t in tr0)            # (from the second iteration on the one-pass kernel itself runs)
    rtol = max(1e-10, 10.0 * max(sens))
    _note(f"graph potential pc567 kind {edge_kind} delta {delta}: the oracle's one-ulp sensitivity {max(sens):.1e}")
    assert max(sens) <= 1e-12                                        # (the comparison below is at 1e-10, not at the oracle's own spread)
    assert _compare_traces(tr, tr0, rtol=rtol) is None
    assert abs(obj[-1] - objr[-1]) <= 1e-11 * abs(objr[-1])
    assert np.linalg.norm(x - xr) <= 1e-10 * np.linalg.norm(xr)


# ---- 9. a size at which a workgroup of the vector launches takes several rounds ------------------------------------------------------------------
@pytest.mark.gpu
def test_edge_eval_at_a_size_of_several_rounds(gpu_lib):
    """A 266 x 266 permuted mesh, n = 70756: a kind-2 refresh with f, grad and diag against numpy float64 with the kernel's expressions.  numpy
    rounds as often as the device does (its bincount adds a row's terms one by one), so every bound of item 2 is taken TWICE: rows within
    2 gamma_{Kr + 7} sum |terms| (grad) and 2 gamma_{Kr + 13} (diag); f against math.fsum of numpy's terms (no summation error on that side) within
    (gamma_{n Kr + 10} + gamma_{10}) f; H through one product with a hash vector v, rows within 2 gamma_{Kr + 14} sum_j |H_ij v_j| (an entry
    carries 14, the fma chain Kr)."""
    import math
    ctx = L.Context(0, gpu_lib)
    try:
        n, ei, ej = _graph("mesh266")
        assert n == 70756
        w, xh = 0.5 + synth.hash_vector(51, len(ei)) ** 2, 2.4 * synth.hash_vector(52, n) - 1.2
        W = L.SparseHessian(ctx, n, ei, ej, w)
        H = W.like()
        kr = W.row_width
        assert kr == 6
        x, g, d = ctx.vector(n, xh), ctx.vector(n), ctx.vector(n)
        f = W.edge_eval(2, DELTA, KAPPA, x, g, d, H)
        assert W.edge_eval(2, DELTA, KAPPA, x) == f                  # (the same reduction from either kernel)
        p0, p1, p2 = (KAPPA * w * p for p in _psi_np(2, xh[ei] - xh[ej], DELTA))
        bc = lambda val, sign=1.0: np.bincount(ei, val, n) + sign * np.bincount(ej, val, n)
        eg = np.abs(g.download() - bc(p1, -1.0)) / bc(np.abs(p1))
        ed = np.abs(d.download() - bc(p2)) / bc(p2)
        f_np = math.fsum(p0.tolist())
        vh = synth.hash_vector(7, n)
        ref = _GraphRef(n, ei, ej, -p2, np.zeros(n))
        eh = np.abs(_mul(ctx, H, vh) - ref._op(vh)) / ref.absrow(vh)
        print(f"[edge eval 70756] grad {eg.max():.2e} (bound {2 * _g(kr + 7):.2e}), diag {ed.max():.2e} ({2 * _g(kr + 13):.2e}), "
              f"f {abs(f - f_np) / f_np:.2e} ({_g(n * kr + 10) + _g(10):.2e}), H v {eh.max():.2e} ({2 * _g(kr + 14):.2e})")
        assert eg.max() <= 2 * _g(kr + 7) and ed.max() <= 2 * _g(kr + 13)
        assert abs(f - f_np) <= (_g(n * kr + 10) + _g(10)) * f_np
        assert eh.max() <= 2 * _g(kr + 14)
    finally:
        ctx.close()
