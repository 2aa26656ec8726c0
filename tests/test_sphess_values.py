"""The structure / values interface of a sparse Hessian: lfpsqp_sphess_map_create / _free / _info, lfpsqp_sphess_set_values and the host layer
above them (SparseHessian.from_pattern, SparsePattern).

The contract is EXACT: every stored slot of both ELL forms becomes the chain sum ((v_p0 + v_p1) + v_p2) ... of its triplets in the order given --
what lfpsqp_sphess_create computes for the same triplets -- so a refreshed handle is compared with a freshly created one bit for bit: entry by
entry through lfpsqp_sphess_mul (the row form; readers of tests/test_sphess_edge.py) and through whole lfpsqp_projcg_sparse solves (the only
observer of the EDGE form: its set-up reads it).  The diagonal output is the in-order host sum of the diagonal triplets (np.add.at), +0.0 where a
row has none, and overwrites.  Graphs come from tests/test_projcg_sparse.py."""
import ctypes as C

import numpy as np
import pytest

import lfpsqp_jl_amd as L
from oracle import synth

from .helpers import POISON, bits
from .test_projcg_diags import _basis
from .test_projcg_sparse import _graph
from .test_sphess_edge import _dense, _entries, _mul


# ---- the triplets --------------------------------------------------------------------------------------------------------------------------
def _u01(seed, n):
    return 0.5 * (synth.hash_vector(seed, n) + 1.0)                   # (hash_vector is uniform on [-1, 1))


def _triplets(n, ei, ej, seed):
    """(rows, cols, vals) in a hashed order: about 10 % of the edges two or three times, about half of all off-diagonal triplets mirrored, about
    10 % of the rows with two diagonal triplets, 70 % with one and 20 % with none.  Off-diagonal values in [-1, -0.3], diagonal ones of both signs."""
    E = len(ei)
    u = _u01(seed, E)
    mult = 1 + (u < 0.10) + (u < 0.04)
    oi, oj = np.repeat(ei, mult), np.repeat(ej, mult)
    flip = _u01(seed + 1, len(oi)) < 0.5
    oi, oj = np.where(flip, oj, oi), np.where(flip, oi, oj)
    u2 = _u01(seed + 2, n)
    dd = np.repeat(np.arange(n), (u2 < 0.8).astype(np.int64) + (u2 < 0.1))
    rows, cols = np.concatenate([oi, dd]), np.concatenate([oj, dd])
    vals = np.concatenate([-(0.3 + 0.7 * _u01(seed + 3, len(oi))), 2.0 * _u01(seed + 4, len(dd)) - 1.0])
    order = np.argsort(_u01(seed + 5, len(rows)), kind='stable')
    return np.ascontiguousarray(rows[order]), np.ascontiguousarray(cols[order]), np.ascontiguousarray(vals[order]), int(mult.max())


def _diag_sum(n, rows, cols, vals):
    want = np.zeros(n)
    sel = rows == cols
    np.add.at(want, rows[sel], vals[sel])                            # (in the order given; 0.0 + v0 = v0 exactly)
    return want


def _same_entries(ctx, name, n, A, B):
    for ea, eb in zip(_entries(ctx, A, name), _entries(ctx, B, name)):          # both triangles
        assert np.array_equal(bits(ea), bits(eb)) and np.all(ea != 0.0)
    if name == "pc567":                                             # ... and nothing outside the pattern
        da = _dense(ctx, A, n)
        _, ei, ej = _graph(name)
        assert np.count_nonzero(da) == 2 * len(ei) and np.array_equal(bits(da), bits(da.T))


# ---- 1. refreshed = created, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pc567", "mesh45", "hub32"])
def test_refreshed_handle_has_the_bits_of_a_created_one(dev_ctx, name):
    ctx = dev_ctx
    n, ei, ej = _graph(name)
    rows, cols, vals, longest = _triplets(n, ei, ej, 60)
    assert longest == 3 and np.any(rows == cols) and np.any(rows > cols) and np.any(rows < cols)
    off = rows != cols
    S, pat = L.SparseHessian.from_pattern(ctx, n, rows, cols)
    created = L.SparseHessian(ctx, n, rows[off], cols[off], vals[off])
    assert (S.n, S.nedges, S.row_width, S.edge_width) == (created.n, created.nedges, created.row_width, created.edge_width)
    assert (pat.nnz, pat.ndiag, pat.max_dup) == (len(rows), int(np.count_nonzero(~off)), 3)          # (4. map_info)
    zero = _mul(ctx, S, synth.hash_vector(7, n))
    assert not np.any(zero)                                         # (created with zero values)
    d = ctx.vector(n).fill(POISON)
    pat.set_values(ctx.vector(len(vals), vals), diag=d, out=S)      # H == S
    _same_entries(ctx, name, n, S, created)
    want = _diag_sum(n, rows, cols, vals)
    got = d.download()
    assert np.array_equal(bits(got), bits(want))
    none = np.bincount(rows[~off], minlength=n) == 0
    assert np.any(none) and np.all(bits(got[none]) == 0)            # +0.0 on rows without a diagonal triplet
    pat.close()
    S.close()
    created.close()


@pytest.mark.parametrize("m,factored", [(4, False), (4, True), (33, False), (33, True)])
@pytest.mark.parametrize("name", ["pc567", "mesh45", "hub32"])
def test_refreshed_handle_solves_bit_for_bit_like_a_created_one(dev_ctx, name, m, factored):
    """A whole lfpsqp_projcg_sparse solve -- its set-up is the only reader of the EDGE form -- on the refreshed handle (here a handle made by like)
    and on the created one: iterates, multipliers, count and nr with equal bits."""
    ctx = dev_ctx
    n, ei, ej = _graph(name)
    rows, cols, vals, _ = _triplets(n, ei, ej, 60)
    off = rows != cols
    S, pat = L.SparseHessian.from_pattern(ctx, n, rows, cols)
    H = S.like()
    pat.set_values(vals, out=H)
    created = L.SparseHessian(ctx, n, rows[off], cols[off], vals[off])
    deg = np.bincount(rows[off], -vals[off], n) + np.bincount(cols[off], -vals[off], n)
    dg = ctx.vector(n, 1.25 * deg + 0.5 + 0.5 * synth.hash_vector(3, n) ** 2)
    b = ctx.vector(n, synth.hash_vector(4, n))
    U, _ = _basis(ctx, n, m, factored)
    work = L.ProjCGWork(ctx, n, m)
    res = []
    for A in (H, created):
        x, lam = ctx.vector(n), ctx.vector(m)
        it, nr = L.projcg_(x, lam, L.SparseOperator(0.0, dg, A), U, b, None, tol=1e-9, work=work)
        res.append((it, nr, x.download(), lam.download()))
    (i0, r0, x0, l0), (i1, r1, x1, l1) = res
    print(f"[set_values] {name} m={m} factored={factored}: {i0} iterations, nr {r0:.3e}")
    assert i0 == i1 and i0 > 3 and bits([r0])[0] == bits([r1])[0]
    assert np.array_equal(bits(x0), bits(x1)) and np.array_equal(bits(l0), bits(l1))


# ---- 2. overwrite, not accumulate ----------------------------------------------------------------------------------------------------------------
def test_values_overwrite_and_leave_everything_else_alone(dev_ctx):
    ctx = dev_ctx
    name = "mesh45"
    n, ei, ej = _graph(name)
    w = 1.5 + synth.hash_vector(51, len(ei))
    W = L.SparseHessian(ctx, n, ei, ej, w)
    H = W.like()
    named = _u01(61, len(ei)) < 0.5
    drow = np.flatnonzero(_u01(62, n) < 0.6)
    rows, cols = np.concatenate([ej[named], drow]), np.concatenate([ei[named], drow])     # (all mirrored: the lower triangle)
    pat = L.SparsePattern(W, rows, cols)
    assert (pat.nnz, pat.ndiag, pat.max_dup) == (len(rows), len(drow), 1)
    k = int(np.count_nonzero(named))
    for seed in (63, 64):
        vals = synth.hash_vector(seed, len(rows)) - 0.5
        vals[vals == 0.0] = 0.25
        pat.set_values(vals, out=H)                                  # (a host array: uploaded into the vector the object keeps)
        for got in _entries(ctx, H, name):
            assert np.array_equal(bits(got[named]), bits(vals[:k])) and np.all(bits(got[~named]) == 0)
    for got in _entries(ctx, W, name):
        assert np.array_equal(bits(got), bits(w))                    # W keeps its values
    want = np.zeros(n)
    want[drow] = vals[k:]
    plain = ctx.vector(n + 3).fill(POISON)
    pat.set_values(vals, diag=plain)                                 # H NULL
    got = plain.download()
    assert np.array_equal(bits(got[:n]), bits(want)) and np.all(bits(got[n:]) == bits([POISON])[0])
    st = L.StackedVector(ctx, n).upload2(np.full(2 * n, POISON))
    before = st.download()
    pat.set_values(vals, diag=st)
    got = st.download()
    assert np.array_equal(bits(got[:n]), bits(want)) and np.array_equal(bits(got[n:]), bits(before[n:]))
    pat.set_values(vals, diag=plain)                                 # a second time: the same, not twice
    assert np.array_equal(bits(plain.download()[:n]), bits(want))


# ---- 3. edge shapes ------------------------------------------------------------------------------------------------------------------------------
def test_one_row_and_no_triplets(dev_ctx):
    ctx = dev_ctx
    S, pat = L.SparseHessian.from_pattern(ctx, 1, [0, 0], [0, 0])   # n = 1: no edges, Kr = Ke = 0; diagonal-only triplets
    assert (S.n, S.nedges, S.row_width, S.edge_width) == (1, 0, 0, 0) and (pat.nnz, pat.ndiag, pat.max_dup) == (2, 2, 2)
    d = ctx.vector(1).fill(POISON)
    pat.set_values(np.array([0.1, 0.7]), diag=d, out=S)
    assert d.download()[0] == 0.1 + 0.7
    assert _mul(ctx, S, np.array([3.0]), 2.0)[0] == 6.0
    S0, pat0 = L.SparseHessian.from_pattern(ctx, 1, [], [])         # nnz = 0
    assert (pat0.nnz, pat0.ndiag, pat0.max_dup) == (0, 0, 0)
    pat0.set_values(ctx.vector(1), diag=d, out=S0)
    assert bits(d.download())[0] == 0
    n, ei, ej = _graph("mesh45")
    W = L.SparseHessian(ctx, n, ei, ej, 1.0)
    H = W.like()
    empty = L.SparsePattern(W, [], [])                              # nnz = 0 over a pattern with edges: everything becomes +0.0
    dn = ctx.vector(n).fill(POISON)
    empty.set_values(np.zeros(0), diag=dn, out=H)
    assert np.all(bits(dn.download()) == 0) and all(np.all(bits(e) == 0) for e in _entries(ctx, H, "mesh45"))
    assert np.all(_entries(ctx, W, "mesh45")[0] == 1.0)


@pytest.mark.parametrize("n", [5, 2047, 2048, 2049])
def test_sizes_around_a_tile(dev_ctx, n):
    """Edges (i, i + 1) and (i, i + 3): i mod 7 is a distance-2 colouring, so seven products read every entry.  Every fifth edge three times, the
    last ones included: chains in the last pair of rows (odd n: the single store) and across the 2048-row boundary.  vals longer than nnz."""
    ctx = dev_ctx
    ei = np.concatenate([np.arange(n - 1), np.arange(n - 3)])
    ej = np.concatenate([np.arange(1, n), np.arange(3, n)])
    mult = np.where(np.arange(len(ei)) % 5 == 3, 3, 1)
    mult[n - 2] = mult[len(ei) - 1] = 3                             # the edges (n - 2, n - 1) and (n - 4, n - 1)
    oi, oj = np.repeat(ei, mult), np.repeat(ej, mult)
    flip = np.arange(len(oi)) % 2 == 1
    oi, oj = np.where(flip, oj, oi), np.where(flip, oi, oj)
    dd = np.concatenate([np.arange(n), np.arange(n - 1, -1, -2)])   # every row once; the last, third from last ... twice
    rows, cols = np.concatenate([oi, dd]), np.concatenate([oj, dd])
    order = np.argsort(synth.hash_vector(70, len(rows)), kind='stable')
    rows, cols = rows[order], cols[order]
    vals = synth.hash_vector(71, len(rows)) - 0.5
    off = rows != cols
    S, pat = L.SparseHessian.from_pattern(ctx, n, rows, cols)
    created = L.SparseHessian(ctx, n, rows[off], cols[off], vals[off])
    assert (S.row_width, S.edge_width, pat.max_dup, pat.ndiag) == (created.row_width, created.edge_width, 3, len(dd))
    H = S.like()
    longer = ctx.vector(len(vals) + 5, np.concatenate([vals, np.full(5, POISON)]))
    d = ctx.vector(n).fill(POISON)
    pat.set_values(longer, out=H)                                   # diag NULL
    assert np.all(bits(d.download()) == bits([POISON])[0])
    pat.set_values(longer, diag=d)                                  # H NULL
    assert np.array_equal(bits(d.download()), bits(_diag_sum(n, rows, cols, vals)))
    for k in range(7):
        e = (np.arange(n) % 7 == k).astype(np.float64)
        got, want = _mul(ctx, H, e), _mul(ctx, created, e)
        assert np.array_equal(bits(got), bits(want)) and (np.any(got != 0.0) or not np.any(e))
    assert not np.any(_mul(ctx, S, synth.hash_vector(7, n)))        # S itself was not the output
    if n >= 2047:                                                   # ... and the edge form, through one solve
        m = 4
        av = np.abs(vals[off])
        dg = ctx.vector(n, np.bincount(rows[off], av, n) + np.bincount(cols[off], av, n) + 0.05 + 0.5 * synth.hash_vector(3, n) ** 2)
        U, _ = _basis(ctx, n, m, False)
        b = ctx.vector(n, synth.hash_vector(4, n))
        res = []
        for A in (H, created):
            x, lam = ctx.vector(n), ctx.vector(m)
            it, nr = L.projcg_(x, lam, L.SparseOperator(0.0, dg, A), U, b, None, tol=1e-9, work=L.ProjCGWork(ctx, n, m))
            res.append((it, bits([nr])[0], bits(x.download()), bits(lam.download())))
        assert res[0][0] == res[1][0] > 3 and res[0][1] == res[1][1]
        assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


# ---- 5. refusals and lifetime ------------------------------------------------------------------------------------------------------------------------
def _setup(ctx):
    n, ei, ej = _graph("pc567")
    W = L.SparseHessian(ctx, n, ei, ej, 1.0)
    rows, cols = np.concatenate([ei, np.arange(n)]), np.concatenate([ej, np.arange(n)])
    return n, ei, ej, W, rows, cols, L.SparsePattern(W, rows, cols)


def test_map_and_set_values_refuse_bad_arguments(dev_ctx):
    ctx = dev_ctx
    n, ei, ej, W, rows, cols, pat = _setup(ctx)
    out = C.c_void_p()

    def create(r, c, S=W, nnz=None):
        r, c = np.ascontiguousarray(r, dtype=np.int64), np.ascontiguousarray(c, dtype=np.int64)
        rc = ctx.L.lfpsqp_sphess_map_create(ctx.h, S.h if S is not None else None, len(r) if nnz is None else nnz, r.ctypes.data, c.ctypes.data,
                                            C.byref(out))
        assert rc == 0 or not out.value
        return rc
    pair = next((a, b) for a in range(n) for b in range(a + 1, n) if not np.any((ei == a) & (ej == b)))
    assert create([ei[0], 3, pair[1]], [ej[0], 3, pair[0]]) == -1   # entry 2 is no edge of the pattern
    msg = ctx.L.lfpsqp_last_error(ctx.h).decode()
    assert "entry 2" in msg and "not an edge" in msg and f"({pair[1]}, {pair[0]})" in msg
    assert create([0, n], [1, 0]) == -1 and "entry 1" in ctx.L.lfpsqp_last_error(ctx.h).decode()
    assert create([-1], [0]) == -1 and create([0], [n]) == -1
    assert create([0], [1], S=None) == -1 and create([0], [1], nnz=-1) == -1
    assert create([0], [1], nnz=2 ** 31) == -5                      # positions are int32 (refused before anything is read)
    assert ctx.L.lfpsqp_sphess_map_info(None, None, None, None) == -1
    assert ctx.L.lfpsqp_sphess_map_free(ctx.h, None) == 0

    H, other = W.like(), L.SparseHessian(ctx, n, ei, ej, 1.0)
    vals, d = ctx.vector(pat.nnz, np.ones(pat.nnz)), ctx.vector(n)

    def call(mm=pat, vv=vals, dd=d, hh=H):
        h = lambda o: None if o is None else o.h
        return ctx.L.lfpsqp_sphess_set_values(ctx.h, h(mm), h(vv), h(dd), h(hh))
    assert call() == 0
    assert call(vv=ctx.vector(pat.nnz - 1)) == -1                   # short vals
    assert call(dd=ctx.vector(n - 1)) == -1                         # short diag
    assert call(dd=vals) == -1                                      # diag aliasing vals
    assert call(hh=other) == -1                                     # the same graph, another pattern object
    assert call(mm=None) == -1 and call(vv=None) == -1
    assert call(hh=W) == 0 and call(dd=None) == 0 and call(hh=None) == 0 and call(dd=None, hh=None) == 0
    assert call(dd=L.StackedVector(ctx, n)) == 0                    # a longer diag is fine
    with pytest.raises(L.LfpsqpError):
        L.SparsePattern(W, [pair[0]], [pair[1]])
    with pytest.raises(ValueError):
        pat.set_values(np.ones(pat.nnz - 1), out=H)


def test_set_values_refuses_row_shards_and_foreign_handles(emu_lib):
    ctx = L.Context(0, emu_lib)
    ctx2 = L.Context(0, emu_lib)
    try:
        n, ei, ej, W, rows, cols, pat = _setup(ctx)
        H2 = L.SparseHessian(ctx2, n, ei, ej, 1.0)
        with pytest.raises(ValueError):
            pat.set_values(np.ones(pat.nnz), out=H2)
        H2.close()
        vals, d, H = ctx.vector(pat.nnz, np.ones(pat.nnz)), ctx.vector(n), W.like()
        assert ctx.L.lfpsqp_sphess_set_values(ctx.h, pat.h, vals.h, d.h, H.h) == 0
        ctx.comm_init_callback(0, 1, lambda ptr, count, op, stream: 0)
        assert ctx.L.lfpsqp_sphess_set_values(ctx.h, pat.h, vals.h, d.h, H.h) == -5
        assert "one rank only" in ctx.L.lfpsqp_last_error(ctx.h).decode()
        assert ctx.L.lfpsqp_sphess_set_values(ctx.h, pat.h, vals.h, None, None) == -5
        with pytest.raises(L.LfpsqpError):
            pat.set_values(vals, out=H)
    finally:
        ctx2.close()
        ctx.close()


@pytest.mark.parametrize("order", ["SMH", "SHM", "MSH", "MHS", "HSM", "HMS"])
def test_map_and_handles_may_be_freed_in_every_order(dev_ctx, order):
    """S (the handle the map was built on), M (the map) and H (a handle made by like) closed in every order; after each close what survives still
    works: a map refreshes a surviving handle to the created bits, a handle still multiplies."""
    ctx = dev_ctx
    name = "hub32"
    n, ei, ej = _graph(name)
    rows, cols, vals, _ = _triplets(n, ei, ej, 80)
    off = rows != cols
    S, M = L.SparseHessian.from_pattern(ctx, n, rows, cols)
    H = S.like()
    created = L.SparseHessian(ctx, n, rows[off], cols[off], vals[off])
    vh = synth.hash_vector(7, n)
    want = bits(_mul(ctx, created, vh))
    alive = {"S": S, "M": M, "H": H}
    scale = 1.0
    for who in order:
        alive.pop(who).close()
        scale *= 0.5                                                # (other values every round: exact scaling, the chain sums scale with it)
        for key, obj in alive.items():
            if key == "M":
                continue
            if "M" in alive:
                d = ctx.vector(n)
                M.set_values(scale * vals, diag=d, out=obj)
                assert np.array_equal(bits(_mul(ctx, obj, vh)), bits(scale * _mul(ctx, created, vh)))
                assert np.array_equal(bits(d.download()), bits(scale * _diag_sum(n, rows, cols, vals)))
            else:
                assert np.all(np.isfinite(_mul(ctx, obj, vh)))
    assert np.array_equal(bits(_mul(ctx, created, vh)), want)
    created.close()
