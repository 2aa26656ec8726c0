"""The matrix-core kernels of the tangent setup (gram_kernel, rmul_kernel, rmul_resident_kernel and the host logic around them:
csrc/factorize.hip, gram_impl / rmul_impl) and the stacked projector products (QtV, QApplyE: csrc/ineq.hip) against exactly
rounded references.

Every reference is computed on the host in integer arithmetic (int64 matrix products) or with `math.fsum` over products that are
exact by construction; floating-point numpy sums and BLAS products are never a reference here.  Integer-valued data: entries of at
most 16 in magnitude and weights from {0, 1, 4, 9} (perfect squares: the kernel's sqrt(w2) is exact), so every product and every
partial sum in any order is an integer far below 2^53, the result does not depend on the summation order and the assertion is ==.

  (a) G = A' diag(w2) A and the extra right-hand columns X over one to four 128-column panels, every border count, ncols < m;
  (b) a single 2^20 at the step and panel edges;
  (c) the same products of views diag(rs) A + u w';
  (d) Out = In W on each of the three rmul kernels;
  (e) (GPU only) row counts at which a workgroup of the full-size grid takes several steps / tiles;
  (f) hostile real data (cancelling sums) against the a-priori bound gamma_k * sum |terms|;
  (g) the weight contract of the header: a negative weight is an argument error;
  (h) lfpsqp_q_gemv_t / _n across widths, lfpsqp_calculate_lambda_y, lfpsqp_augmented_diag, lfpsqp_ineq_rhs.

Each case runs on the CPU emulator build and, under -m gpu, on the MI355X, with the same assertions."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import lfpsqp_jl_amd as L
from tests.helpers import POISON, bits, gamma, i64, imatmul, ints, short_reals

BIG = 2.0 ** 20                                  # the sentinel
SQUARES = np.array([0.0, 1.0, 4.0, 9.0])
LIM = 16                                         # |entries| of the integer matrices


def weights(seed, n):
    """Perfect squares from {0, 1, 4, 9} (about a quarter of the rows get the weight zero)."""
    return SQUARES[np.random.default_rng(seed).integers(0, 4, n)]


def poisoned(Mh, ncols):
    out = np.array(Mh, order="F")
    out[:, ncols:] = np.nan
    return out


# ================================================================================================================================
# (a) Gram, exact
# ================================================================================================================================
# 1 .. 4 panels; beyond a multiple of 128: 1, 2, 4 border columns (129, 130, 132; 257, 260; 385, 388) and 5 = no border but one panel
# more (133, 261, 389); with nx = 0, 1, 2 columns of the caller's, min(border, 2 - nx) border columns ride with the pass and the others
# take GEMV-T passes.  ncols = m - 1 and m - 3 reach the neighbouring border counts and the non-full last panel under NaN columns.
GRAM_M = [1, 4, 5, 33, 127, 128, 129, 130, 132, 133, 256, 257, 260, 261, 385, 388, 389]
GRAM_CASES = [(n, m) for n in (17, 2049) for m in GRAM_M] + [(n, m) for n in (1, 15, 129, 700) for m in (5, 128, 130, 133, 261)]


@functools.lru_cache(maxsize=8)
def _gram_data(n, m):
    """(M, w2, sqrt(w2), E) and the int64 references for all m columns: (G, X) unweighted and weighted.  The Gram matrix of the leading
    ncols columns is the leading block of G.  e_0 is 2^20 in the rows of weight zero: they must drop out of the weighted X."""
    Mh = np.asfortranarray(ints(1000 * m + n, (n, m), LIM))
    w2h = weights(n + m, n)
    Eh = np.stack([ints(n + m + 1, n, LIM), ints(n + m + 2, n, LIM)], axis=1)
    Eh[w2h == 0.0, 0] = BIG
    Mi, wi, Ei = i64(Mh), i64(w2h), i64(Eh)
    si = i64(np.sqrt(w2h))
    assert np.array_equal(si * si, wi)
    ref = {False: (imatmul(Mi.T, Mi), imatmul(Mi.T, Ei)),
           True: (imatmul((Mi * wi[:, None]).T, Mi), imatmul(Mi.T, Ei * si[:, None]))}
    for v in (Mh, w2h, Eh):
        v.setflags(write=False)
    return Mh, w2h, Eh, ref


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("cut", [0, 1, 3])
@pytest.mark.parametrize("n,m", GRAM_CASES)
def test_gram_is_exact_on_integer_data(dev_ctx, n, m, cut, weighted):
    """lfpsqp_gram and lfpsqp_gram_rhs (nx = 1, 2), weighted and not, for ncols = m, m - 1, max(m - 3, 1) (cut = 0, 1, 3; a case
    apiece: an emulated pass over four panels of 2049 rows takes 0.8 s): G == the int64 product,
    X == M'(sqrt(w2) .* e_k), G is symmetric bit for bit, gram_rhs's G has the bits of gram's.  The columns >= ncols of the matrix are
    NaN and must not reach either; about a quarter of the weights are exactly zero and those rows drop out (e_0 is 2^20 there).
    n = 1, 15, 17: one ragged 16-row step and a step edge with one row either side; 129, 700, 2049: several steps, the last ragged."""
    ctx = dev_ctx
    Mh, w2h, Eh, ref = _gram_data(n, m)
    M, w2 = ctx.matrix(n, m), ctx.vector(n, w2h)
    es = [ctx.vector(n, Eh[:, 0]), ctx.vector(n, Eh[:, 1])]
    ncols = max(m - 3, 1) if cut == 3 else m - cut
    M.upload(poisoned(Mh, ncols))
    Gref, Xref = ref[weighted]
    w = w2 if weighted else None
    G0 = L.gram(M, ncols, w)
    assert np.array_equal(G0, Gref[:ncols, :ncols]), ncols
    assert np.array_equal(G0, G0.T)
    for nx in (1, 2):
        G, X = L.gram_rhs(M, es[:nx], ncols, w)
        assert np.array_equal(bits(G), bits(G0)), (ncols, nx)
        assert np.array_equal(X, Xref[:ncols, :nx]), (ncols, nx)
    for o in (M, w2, *es):
        o.free()


# ================================================================================================================================
# (b) Gram, a single large entry
# ================================================================================================================================
@pytest.mark.parametrize("ncols", [130, 261])
@pytest.mark.parametrize("p", [0, 15, 16, 17, -1])
def test_gram_single_large_entry(dev_ctx, ncols, p):
    """All zeros but 2^20 in row p (the first and the last row, a step edge and one row either side) of the columns i and j, from
    {0, 127, 128, ncols - 1} (panel edges, the border columns of ncols = 130, the short third panel of 261): G is w_p 2^40 at (i, i),
    (i, j), (j, i), (j, j) and 0 elsewhere, X picks sqrt(w_p) e_p.  Column ncols, one past the count, holds the same entry all the time
    and reaches nothing.  Every other pair runs weighted (w_p = 9)."""
    ctx = dev_ctx
    n, m = 700, ncols + 1
    p %= n
    col = np.zeros((n, 1))
    col[p] = BIG
    M = ctx.matrix(n, m)
    M.upload(col, ncols)
    eh = ints(ncols + p, n, LIM)
    eh[p] = -7.0
    w2h = weights(p, n)
    w2h[p] = 9.0
    e, w2 = ctx.vector(n, eh), ctx.vector(n, w2h)
    spots = [0, 127, 128, ncols - 1]
    pairs = [(i, j) for a, i in enumerate(spots) for j in spots[a:]]
    for k, (i, j) in enumerate(pairs):
        weighted = k % 2 == 1
        for c in {i, j}:
            M.upload(col, c)
        G, X = L.gram_rhs(M, [e], ncols, w2 if weighted else None)
        Gref, Xref = np.zeros((ncols, ncols)), np.zeros((ncols, 1))
        for a in (i, j):
            Xref[a] = (3.0 if weighted else 1.0) * BIG * eh[p]
            for b in (i, j):
                Gref[a, b] = (9.0 if weighted else 1.0) * BIG * BIG
        assert np.array_equal(G, Gref), (i, j, weighted)
        assert np.array_equal(X, Xref), (i, j, weighted)
        for c in {i, j}:
            M.upload(np.zeros((n, 1)), c)
    for o in (M, e, w2):
        o.free()


# ================================================================================================================================
# (c) Gram on views, exact
# ================================================================================================================================
def _view_case(ctx, n, m, seed):
    """A, rs (an exact zero in row 0, both signs), u, w as integers and on the device."""
    Ah = np.asfortranarray(ints(seed, (n, m), LIM))
    rsh, uh, wh = ints(seed + 1, n, 3), ints(seed + 2, n, 4), ints(seed + 3, m, 4)
    rsh[:3] = [0.0, -2.0, 3.0]
    return Ah, rsh, uh, wh, ctx.matrix(n, m, Ah), ctx.vector(n, rsh), ctx.vector(n, uh), ctx.vector(m, wh)


def _view_forms(A, rs, u, w, Ah, rsh, uh, wh):
    """(view, the materialised int64 matrix) for diag(rs) A, A + u w', diag(rs) A + u w'."""
    Ai, ri, uw = i64(Ah), i64(rsh), np.outer(i64(uh), i64(wh))
    return [(A.view(rs=rs), ri[:, None] * Ai), (A.view(u=u, w=w), Ai + uw), (A.view(rs=rs, u=u, w=w), ri[:, None] * Ai + uw)]


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("n", [17, 513, 2049])
@pytest.mark.parametrize("m", [5, 128, 131, 260])
def test_gram_on_views_is_exact(dev_ctx, n, m, form):
    """V = diag(rs) A + u w' (form 0: rs only, 1: the rank-one term only, 2: both): V' diag(w2) V and V'(sqrt(w2) .* e_k) == the int64 products of
    the materialised matrix, weighted and not, nx = 0, 1, 2 -- at nx = 2 the rank-one column z no longer rides with the pass and takes
    the GEMV-T branch; m = 131 and 260 add 3 and 4 border columns under the view."""
    ctx = dev_ctx
    Ah, rsh, uh, wh, A, rs, u, w = _view_case(ctx, n, m, 77 * m + n)
    w2h = weights(n + m + 5, n)
    Eh = np.stack([ints(n + m + 6, n, LIM), ints(n + m + 7, n, LIM)], axis=1)
    wi, si, Ei = i64(w2h), i64(np.sqrt(w2h)), i64(Eh)
    w2, es = ctx.vector(n, w2h), [ctx.vector(n, Eh[:, 0]), ctx.vector(n, Eh[:, 1])]
    V, Vi = _view_forms(A, rs, u, w, Ah, rsh, uh, wh)[form]
    for weighted in (False, True):
        Gref = imatmul((Vi * wi[:, None]).T if weighted else Vi.T, Vi)
        Xref = imatmul(Vi.T, Ei * si[:, None] if weighted else Ei)
        for nx in (0, 1, 2):
            if nx == 0:
                G = L.gram(V, m, w2 if weighted else None)
            else:
                G, X = L.gram_rhs(V, es[:nx], m, w2 if weighted else None)
                assert np.array_equal(X, Xref[:, :nx]), (weighted, nx)
            assert np.array_equal(G, Gref), (weighted, nx)
            assert np.array_equal(G, G.T)
    assert np.array_equal(A.download(), Ah)


# ================================================================================================================================
# (d) rmul, exact, all three kernels
# ================================================================================================================================
RMUL_K = [1, 3, 4, 16, 17, 127, 128, 129, 132, 133, 257]
RMUL_R = [1, 5, 128, 129, 144, 145, 255]
RMUL_N = [1, 17, 129, 700]


def _check_rmul(ctx, In, Ii, k, r, seed):
    """Out (r + 2 columns, poisoned) = In[:, :k] W: the leading r columns == the int64 product, the others keep their bits."""
    n = Ii.shape[0]
    Wh = ints(seed, (k, r), LIM)
    Out = ctx.matrix(n, r + 2, np.full((n, r + 2), POISON, order="F"))
    L.rmul(In, Wh, Out)
    got = Out.download()
    assert np.array_equal(got[:, :r], imatmul(Ii[:, :k], i64(Wh))), (n, k, r)
    assert np.array_equal(bits(got[:, r:]), bits(np.full((n, 2), POISON))), (n, k, r)
    Out.free()


@pytest.mark.parametrize("k", RMUL_K)
def test_rmul_is_exact_on_integer_data(dev_ctx, k):
    """lfpsqp_rmul for k input and r output columns.  rmul_impl picks the kernel by shape: k <= 128 and r <= 128 -- rmul_resident_kernel
    <32, 8, 16> (W resident in LDS, persistent grid); else k <= 132 and r <= 144 -- the wider resident form <33, 9, 11> (k = 129, 132 with
    any r <= 144, and k <= 128 with r = 129, 144); anything else (k = 133, 257, or r = 145, 255) -- rmul_kernel.  n = 1, 17, 129: a ragged
    first tile and a second tile of one row; n = 700: six tiles, so that a workgroup of the emulator's 4-CU persistent grid walks two.
    Column k of In is NaN and must not be read into the result; In comes back bit for bit."""
    ctx = dev_ctx
    for n in RMUL_N:
        Inh = np.asfortranarray(ints(31 * k + n, (n, k + 1), LIM))
        Ii = i64(Inh)
        Inh[:, k] = np.nan
        In = ctx.matrix(n, k + 1, Inh)
        for r in RMUL_R:
            _check_rmul(ctx, In, Ii, k, r, 7 * k + r + n)
        assert np.array_equal(bits(In.download()), bits(Inh))
        In.free()


@pytest.mark.parametrize("k,r", [(128, 128), (132, 144), (133, 145)])
def test_rmul_with_the_resident_kernels_switched_off(dev_ctx, k, r):
    """lfpsqp_ctx_set_onepass(-1) (rmul_impl tests tune_onepass >= 0 before either resident form): rmul_kernel at one shape of each
    kernel, with the same exact result."""
    ctx = dev_ctx
    ctx.set_onepass(-1)
    try:
        for n in (129, 700):
            Inh = np.asfortranarray(ints(k + n, (n, k + 1), LIM))
            Ii = i64(Inh)
            Inh[:, k] = np.nan
            In = ctx.matrix(n, k + 1, Inh)
            _check_rmul(ctx, In, Ii, k, r, k + r)
            In.free()
    finally:
        ctx.set_onepass(0)


def test_rmul_of_a_view_is_exact(dev_ctx):
    """(diag(rs) A + u w')[:, :k] W at (513, 131): the product over the plain storage, then view_rows_kernel; k = 128 (resident),
    131 (wider resident), and r = 150 (rmul_kernel)."""
    ctx = dev_ctx
    n, m = 513, 131
    Ah, rsh, uh, wh, A, rs, u, w = _view_case(ctx, n, m, 4242)
    V, Vi = _view_forms(A, rs, u, w, Ah, rsh, uh, wh)[2]
    for k, r in ((131, 131), (128, 5), (131, 150)):
        _check_rmul(ctx, V, Vi, k, r, k + r)
    assert np.array_equal(A.download(), Ah)


# ================================================================================================================================
# (e) GPU only: the multi-step paths of the full-size grids
# ================================================================================================================================
PERIOD = 1021                                    # prime: the 16-row steps and 128-row tiles meet every alignment of the base block


def _periodic_rows(seed, n, cols):
    """Row r of the matrix is c_r * B[r mod PERIOD] with |B| <= 5 and c_r from {-3 .. 3} \\ {0}: |entries| <= 15, and products with
    the n-row matrix reduce to int64 products with the PERIOD-row block B (the references of (e) stay cheap on the host)."""
    rng = np.random.default_rng(seed)
    B = rng.integers(-5, 6, (PERIOD, cols))
    c = rng.choice(np.array([-3, -2, -1, 1, 2, 3]), n)
    q = np.arange(n) % PERIOD
    Mh = np.empty((n, cols), order="F")
    for j in range(cols):
        Mh[:, j] = c * B[q, j]
    return Mh, B, c, q


def _fold(q, values):
    """sum of `values` over the rows of each residue class (int64)."""
    out = np.zeros(PERIOD, dtype=np.int64) if values.ndim == 1 else np.zeros((PERIOD, values.shape[1]), dtype=np.int64)
    np.add.at(out, q, values)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("m", [128, 130, 260, 385])
def test_gram_multi_step_groups_are_exact(gpu_lib, m):
    """n = 16 * (3 * 512 + 5) + 3 = 24659 rows: nsteps = 1542 16-row steps, the last of 3 rows.  gram_impl launches
    groups_for(np) = (2 * num_cu / np) / 8 * 8 row groups for a launch of np panel pairs (capped by the steps rounded up to 8); a group
    takes the steps g, g + groups, ...  On 256 CUs: one panel (m = 128; 130 = 128 + 2 border columns) -- 512 groups, 3 or 4 steps each;
    m = 260 (two panels + 4 border columns) -- 256 groups of 6 or 7 steps for the two diagonal pairs, 512 of 3 or 4 for the
    off-diagonal pair; m = 385 (three panels + 1) -- 512 / 3 / 8 * 8 = 168 groups of 9 or 10 steps in both launches.  At n <= 8192
    every group has at most one step and the double-buffered loop of gram_kernel never turns.  Weighted with nx = 2 and unweighted
    with nx = 0, == the int64 reference (rows c_r * B[r mod 1021]: G = B' diag(d) B with d_q the sum of w_r c_r^2 over the class)."""
    ctx = L.Context(0, gpu_lib)
    try:
        n = 16 * (3 * 512 + 5) + 3
        steps = (n + 15) // 16
        for np_, lo in ((1, 3), (2, 6), (3, 9)):
            groups = min(512 // np_ // 8 * 8, (steps + 7) // 8 * 8)
            assert steps // groups == lo and steps % groups != 0 and n % 16 == 3
        Mh, B, c, q = _periodic_rows(m, n, m)
        w2h = weights(m + 1, n)
        Eh = np.stack([ints(m + 2, n, LIM), ints(m + 3, n, LIM)], axis=1)
        wi, si, Ei = i64(w2h), i64(np.sqrt(w2h)), i64(Eh)
        M, w2 = ctx.matrix(n, m, Mh), ctx.vector(n, w2h)
        es = [ctx.vector(n, Eh[:, 0]), ctx.vector(n, Eh[:, 1])]
        G = L.gram(M, m, None)
        assert np.array_equal(G, imatmul((B * _fold(q, c * c)[:, None]).T, B))
        assert np.array_equal(G, G.T)
        G, X = L.gram_rhs(M, es, m, w2)
        assert np.array_equal(G, imatmul((B * _fold(q, wi * c * c)[:, None]).T, B))
        assert np.array_equal(X, imatmul(B.T, _fold(q, (c * si)[:, None] * Ei)))
        assert np.array_equal(G, G.T)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k,r", [(128, 128), (132, 130), (260, 257)])
def test_rmul_multi_tile_workgroups_are_exact(gpu_lib, k, r):
    """n = 128 * (2 * 256 + 3) + 5 = 65925 rows: 516 tiles of 128 rows, the last of 5.  The persistent grid of rmul_resident_kernel is
    pgrid = min(tiles, num_cu) workgroups with a contiguous balanced span of tiles each: on 256 CUs 516 = 2 * 256 + 4 -- workgroups 0 .. 3
    walk three tiles, the others two (below n = 32768 every workgroup has one tile and the register ring never crosses a tile edge).
    (128, 128): resident; (132, 130): the wider resident form; (260, 257): rmul_kernel, 520 * 3 workgroups.  Out (poisoned, two
    columns more) == the int64 product (row r of In is c_r * B[r mod 1021]: row r of the product is c_r * (B W)[r mod 1021])."""
    ctx = L.Context(0, gpu_lib)
    try:
        n = 128 * (2 * 256 + 3) + 5
        tiles = (n + 127) // 128
        assert tiles // 256 == 2 and tiles % 256 == 4 and n % 128 == 5
        Inh, B, c, q = _periodic_rows(k + r, n, k)
        Wh = ints(k * r, (k, r), LIM)
        In = ctx.matrix(n, k, Inh)
        Out = ctx.matrix(n, r + 2)
        for j in range(r + 2):
            Out.upload(np.full((n, 1), POISON), j)
        L.rmul(In, Wh, Out)
        BW = imatmul(B, i64(Wh))
        for j0 in range(0, r + 2, 64):                                   # (in slabs: the whole matrix twice over is 270 MB of host memory)
            got = Out.download(j0, min(64, r + 2 - j0))
            for j in range(j0, j0 + got.shape[1]):
                if j < r:
                    assert np.array_equal(got[:, j - j0], c * BW[q, j]), j
                else:
                    assert np.array_equal(bits(got[:, j - j0]), bits(np.full(n, POISON))), j
    finally:
        ctx.close()


# ================================================================================================================================
# (f) rounding-error bounds on cancelling data
# ================================================================================================================================
def _fsum_columns(P):
    """math.fsum of every column of P (whose entries are exact products)."""
    return np.array([math.fsum(col) for col in np.ascontiguousarray(P.T).tolist()])


@functools.lru_cache(maxsize=2)
def _cancelling_gram_case(n, m, weighted):
    """M and s = sqrt(w2) with 13-bit mantissas: w2 = s^2 (26 bits) and w2 * M_ri * M_rj (52 bits) are exact, math.fsum of the products
    is the true entry (rounded once) .  The lower half of the rows mirrors the upper half with column j multiplied by a random sign
    s_j: G_ij = (1 + s_i s_j) * (the sum over the upper half) + the unpaired row of an odd n, so about half of the entries cancel to that
    one term (2^-60; zero for an even n).  Returns (M, w2, exact, mag) for the upper triangle, mag = sum_r |w_r M_ri M_rj|
    rounded DOWN (a numpy sum of non-negative exact terms, lowered by 2^-40 relative: its own rounding error is below n 2^-53)."""
    rng = np.random.default_rng(n * m)
    h = n // 2
    top = np.stack([short_reals(1000 * j + n, h, -10, 10, 13) for j in range(m)], axis=1)
    sign = rng.choice([-1.0, 1.0], m)
    st = np.abs(short_reals(n + m, h, -5, 5, 13))
    perm = rng.permutation(n)
    Mh = np.asfortranarray(np.concatenate([top, top * sign[None, :], np.ldexp(np.ones((n - 2 * h, m)), -30)])[perm])
    sw = np.concatenate([st, st, np.ones(n - 2 * h)])[perm]
    w2h = sw * sw
    exact, mag = np.zeros((m, m)), np.zeros((m, m))
    for i in range(m):
        P = ((w2h * Mh[:, i]) if weighted else Mh[:, i])[:, None] * Mh[:, i:]
        exact[i, i:] = _fsum_columns(P)
        mag[i, i:] = np.abs(P).sum(axis=0) * (1.0 - 2.0 ** -40)
    return Mh, w2h, exact, mag


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,m", [(1025, 37), (2049, 130), (700, 261)])
def test_gram_error_bound_on_cancelling_data(dev_ctx, n, m, weighted):
    """|G_ij - exact| <= gamma_k * sum_r |w_r M_ri M_rj| for every entry.
    Unweighted, k = n + 1: the n products are exact or fused into the accumulation (matrix-core instruction, fma of the riding border
    columns and of the GEMV-T passes), and a term then passes through at most n - 1 additions in whatever order the k-groups, steps,
    row groups and the reduction of the partials take them: n - 1 roundings, + 1 for a product rounded on its own, + 1 spare for the
    additions of a zero-initialised accumulator.
    Weighted, k = n + 5: each of the two operands is fl(fl(sqrt(w_r)) * M_r.), two roundings a side = 4 more (the GEMV-T passes of the
    border columns use fl(w_r * M_rj) on one side: fewer).  The host's symmetrisation 0.5 * (G_ij + G_ji) is exact: both triangles
    hold the same value, mirrored or copied (gram_impl).  Three panels with a short last one, one panel + 2 border columns, a
    single short panel.  At least a third of the entries have |exact| <= 1e-10 * mag, so the data stays hostile."""
    ctx = dev_ctx
    Mh, w2h, exact, mag = _cancelling_gram_case(n, m, weighted)
    M, w2 = ctx.matrix(n, m, Mh), ctx.vector(n, w2h)
    iu = np.triu_indices(m)
    G = L.gram(M, m, w2 if weighted else None)
    assert np.array_equal(G, G.T)
    k = n + 5 if weighted else n + 1
    share = np.mean(np.abs(exact[iu]) <= 1e-10 * mag[iu])
    ratios = [float(abs(Fraction(g) - Fraction(e)) / (gamma(k) * Fraction(b))) for g, e, b in zip(G[iu].tolist(), exact[iu].tolist(), mag[iu].tolist())]
    print(f"gram n={n} m={m} weighted={weighted}: worst |err| / bound = {max(ratios):.4f} (k = {k}), cancelling share = {share:.3f}")
    assert share >= 1.0 / 3.0
    assert max(ratios) <= 1.0, int(np.argmax(ratios))


@pytest.mark.parametrize("k,r", [(127, 128), (131, 140), (257, 130)])
def test_rmul_error_bound_on_cancelling_data(dev_ctx, k, r):
    """Out[i, c] = sum_j In[i, j] W[j, c], per entry: k products (exact: both factors have 26 significant bits; fused into the
    accumulation anyway) and at most k - 1 additions in the order of the k-groups, + 1 spare: |computed - exact| <= gamma_{k+1} *
    sum_j |In_ij W_jc|.  The right half of In's columns repeats the left half and the lower half of W's rows is the upper half times a
    random sign per output column: about half of the output columns cancel to the unpaired term 2^-60.  One shape per kernel:
    resident, the wider resident form, rmul_kernel."""
    ctx = dev_ctx
    n, h = 300, k // 2
    rng = np.random.default_rng(k * r)
    left = np.stack([short_reals(77 * j + k, n, -10, 10) for j in range(h)], axis=1)
    Wt = np.stack([short_reals(55 * c + r, h, -10, 10) for c in range(r)], axis=1)
    sign = rng.choice([-1.0, 1.0], r)
    perm = rng.permutation(k)
    Inh = np.asfortranarray(np.concatenate([left, left, np.ldexp(np.ones((n, k - 2 * h)), -30)], axis=1)[:, perm])
    Wh = np.asfortranarray(np.concatenate([Wt, Wt * sign[None, :], np.ldexp(np.ones((k - 2 * h, r)), -30)])[perm])
    In, Out = ctx.matrix(n, k, Inh), ctx.matrix(n, r)
    L.rmul(In, Wh, Out)
    got = Out.download()
    worst, cancelled = 0.0, 0
    g = gamma(k + 1)
    for i in range(n):
        P = Inh[i, :, None] * Wh                                         # k x r exact products
        exact, mag = _fsum_columns(P), np.abs(P).sum(axis=0) * (1.0 - 2.0 ** -40)
        cancelled += int(np.sum(np.abs(exact) <= 1e-10 * mag))
        err = [abs(Fraction(a) - Fraction(b)) for a, b in zip(got[i].tolist(), exact.tolist())]
        worst = max(worst, max(float(e / (g * Fraction(b))) for e, b in zip(err, mag.tolist())))
    print(f"rmul k={k} r={r}: worst |err| / bound = {worst:.4f} (k = {k + 1}), cancelling share = {cancelled / (n * r):.3f}")
    assert cancelled >= n * r / 3
    assert worst <= 1.0


# ================================================================================================================================
# (g) the documented weight contract
# ================================================================================================================================
@pytest.mark.parametrize("m", [5, 130])
def test_a_negative_weight_is_an_argument_error(dev_ctx, m):
    """include/lfpsqp_hip.h: "a negative weight is answered with LFPSQP_ERR_ARG (lfpsqp_gram / _gram_rhs) ... never with NaN data" --
    one negative weight in row 0, in row n - 1 and in a middle step; the next valid call on the same context returns the exact G."""
    ctx = dev_ctx
    n = 700
    Mh = np.asfortranarray(ints(m, (n, m), LIM))
    w2h = weights(m + 1, n)
    eh = ints(m + 2, n, LIM)
    Mi, wi = i64(Mh), i64(w2h)
    Gref = imatmul((Mi * wi[:, None]).T, Mi)
    M, w2, e = ctx.matrix(n, m, Mh), ctx.vector(n, w2h), ctx.vector(n, eh)
    for row in (0, n - 1, 16 * 20 + 5):
        w2.upload(np.array([-4.0]), row)
        with pytest.raises(L.LfpsqpError):
            L.gram(M, m, w2)
        with pytest.raises(L.LfpsqpError):
            L.gram_rhs(M, [e], m, w2)
        w2.upload(w2h[row:row + 1], row)
        assert np.array_equal(L.gram(M, m, w2), Gref)
        G, X = L.gram_rhs(M, [e], m, w2)
        assert np.array_equal(G, Gref) and np.array_equal(X[:, 0], imatmul(Mi.T, i64(np.sqrt(w2h)) * i64(eh)))


# ================================================================================================================================
# (h) the stacked projector products across widths, and the elementwise pieces next to them
# ================================================================================================================================
def _nonfinite(n):
    bad = np.full(n, np.nan)
    bad[1::3], bad[2::3] = np.inf, -np.inf
    return bad


@pytest.mark.parametrize("N", [1, 2, 513, 2049])
@pytest.mark.parametrize("m", [0, 1, 7, 8, 9, 255, 256, 257])
def test_stacked_projector_products_are_exact(dev_ctx, N, m):
    """lfpsqp_q_gemv_t / _n through InequalityDecompProject.mul_t / mul_n for Q = [[diag Dx; diag Dy], [sx; sy] .* Z[:, :rank]] on
    integer data, rank = m - 2: m = 255 .. 257 reach the 256-column chunk of the GEMV kernels, 7 .. 9 the column-unroll tails, 0 and 1
    the empty basis.  With the default tuning and with lfpsqp_ctx_set_tuning(4, 1); with the basis as Z and in factored form (Z = None,
    Z = Jct W[:, :rank]).
      mul_t: w == Dx vx + Dy vy, t[:rank] == Z'(sx vx + sy vy); t[rank:] keeps its poison.
      mul_n: y == alpha [Dx w + sx (Z t); Dy w + sy (Z t)] + beta y for (alpha, beta) in (2, -3), (1, 0), (-1, 1), (3, 0), w given and
             None; t[rank:] is NaN and unread; with beta == 0, y is full of NaN and Inf on input; the gap [N, hs) stays zero."""
    ctx = dev_ctx
    rank = max(m - 2, 0)
    seed = 1000 * m + N
    Ah = np.asfortranarray(ints(seed, (N, m), 8))
    Wh = np.asfortranarray(ints(seed + 1, (m, m), 2))
    Dh = {name: ints(seed + 2 + k, N, 8) for k, name in enumerate(("Dx", "Dy", "sx", "sy"))}
    vh, wh, yh, th = ints(seed + 6, 2 * N, 8), ints(seed + 7, N, 8), ints(seed + 8, 2 * N, 8), ints(seed + 9, max(m, 1), 8)
    Di = {k: i64(v) for k, v in Dh.items()}
    vi, wi, yi, ti = i64(vh), i64(wh), i64(yh), i64(th)
    A = ctx.matrix(N, m, Ah if m else None)
    v, w, y = L.StackedVector(ctx, N).upload2(vh), ctx.vector(N, wh), L.StackedVector(ctx, N)
    tt = th.copy()
    tt[rank:] = np.nan
    t_in, t_out, w_out = ctx.vector(max(m, 1), tt), ctx.vector(max(m, 1)), ctx.vector(N)
    hs = y.hs
    try:
        for ks in (0, 4):
            ctx.set_tuning(ks, True)
            for factored in (False, True):
                Zi = imatmul(i64(Ah), i64(Wh)[:, :rank]) if factored else i64(Ah)[:, :rank]
                if factored:
                    idc = L.InequalityDecomp(ctx, N, m, Jct=A, factored=True)
                    idc.W = Wh
                else:
                    idc = L.InequalityDecomp(ctx, N, m, Jct=A, Z=A)
                idc.rank = rank
                for name in Dh:
                    getattr(idc, name).upload(Dh[name])
                P = L.InequalityDecompProject(idc)
                where = (N, m, ks, factored)
                # Q'v
                t_out.fill(POISON); w_out.fill(POISON)
                P.mul_t(w_out, t_out, v)
                assert np.array_equal(w_out.download(), Di["Dx"] * vi[:N] + Di["Dy"] * vi[N:]), where
                got = t_out.download()
                assert np.array_equal(got[:rank], imatmul(Zi.T, Di["sx"] * vi[:N] + Di["sy"] * vi[N:])), where
                assert np.array_equal(bits(got[rank:]), bits(np.full(got.size - rank, POISON))), where
                # Q [w; t]
                acc = imatmul(Zi, ti[:rank])
                for alpha, beta in ((2, -3), (1, 0), (-1, 1), (3, 0)):
                    for with_w in (True, False):
                        y.upload2(yh if beta else _nonfinite(2 * N))
                        P.mul_n(y, w if with_w else None, t_in, alpha, beta)
                        ox = Di["sx"] * acc + (Di["Dx"] * wi if with_w else 0)
                        oy = Di["sy"] * acc + (Di["Dy"] * wi if with_w else 0)
                        ref = alpha * np.concatenate([ox, oy]) + (beta * yi if beta else 0)
                        assert np.array_equal(y.download2(), ref), (where, alpha, beta, with_w)
                        assert not y.download(hs - N, N).any(), (where, alpha, beta, with_w)
        assert np.array_equal(bits(t_in.download()), bits(tt))
        if m:
            assert np.array_equal(A.download(), Ah)
    finally:
        ctx.set_tuning(0, True)


@pytest.mark.parametrize("N,m", [(1, 2), (2, 5), (513, 9), (2049, 130)])
def test_lambda_y_augmented_diag_and_ineq_rhs_are_exact(dev_ctx, N, m):
    """The formulas of include/lfpsqp_hip.h on integer data, ==:
      lfpsqp_calculate_lambda_y   lamy = (-Dx .* (Jct[:, :ncols] lam) + w) ./ S with S from the powers of two 1/4 .. 4 (the quotients are
                                  exact); ncols = m - 1, the column beyond and lam's tail are NaN and unread;
      lfpsqp_augmented_diag       a = [hx + 2 lamy .* q; 2 lamy .* s] for all four kinds of bound; the gap of the stacked a stays zero;
      lfpsqp_ineq_rhs             e[:N] = |Dy| .* dx - Dx .* sgn(Dy) .* dy with some Dy exactly +0 and -0 (sgn = 0: the dy term drops);
                                  e is longer than N and its tail keeps its poison."""
    ctx = dev_ctx
    rng = np.random.default_rng(N + m)
    ncols = m - 1
    Jh = np.asfortranarray(ints(N * m, (N, m), LIM))
    Ji = i64(Jh)[:, :ncols]
    Jct = ctx.matrix(N, m, poisoned(Jh, ncols))
    lamh = ints(N + m + 1, m, 8)
    lami = i64(lamh)[:ncols]
    lamh[ncols:] = np.nan
    Dxh, wh = ints(N + 2, N, 8), ints(N + 3, N, 64)
    Sh = np.ldexp(1.0, rng.integers(-2, 3, N))
    lamy = ctx.vector(N, np.full(N, POISON))
    lam, Dx, S, w = ctx.vector(m, lamh), ctx.vector(N, Dxh), ctx.vector(N, Sh), ctx.vector(N, wh)
    ctx.check(ctx.L.lfpsqp_calculate_lambda_y(ctx.h, Jct.h, ncols, lam.h, Dx.h, S.h, w.h, lamy.h))
    num = i64(wh) - i64(Dxh) * imatmul(Ji, lami)
    assert np.array_equal(lamy.download(), num.astype(np.float64) / Sh)               # (a division by a power of two: exact)
    # augmented diagonal: kinds none / lower / upper / both  ->  (q, s) = (0, 0), (0, -1), (0, 1), (1, 1)
    kind = np.arange(N) % 4
    xl = np.where((kind == 1) | (kind == 3), -1.0, -np.inf)
    xu = np.where((kind == 2) | (kind == 3), 2.0, np.inf)
    qi, si = np.array([0, 0, 0, 1])[kind], np.array([0, -1, 1, 1])[kind]
    idata = L.InequalityData(ctx, xl, xu)
    hxh, lyh = ints(N + 4, N, LIM), ints(N + 5, N, LIM)
    a = L.StackedVector(ctx, N)
    hx, ly = ctx.vector(N, hxh), ctx.vector(N, lyh)
    L.augmented_hess_diag_(a, hx, ly, idata)
    assert np.array_equal(a.download2(), np.concatenate([i64(hxh) + 2 * i64(lyh) * qi, 2 * i64(lyh) * si]))
    assert not a.download(a.hs - N, N).any()
    # the right-hand column of the bound-stacked projection
    Dyh, dh = ints(N + 6, N, 8), ints(N + 7, 2 * N, 8)
    Dyh[Dyh == 0.0] = np.where(rng.random(int(np.sum(Dyh == 0.0))) < 0.5, 0.0, -0.0)
    Dyh[0] = -0.0
    if N > 1:
        Dyh[1] = 0.0
    d = L.StackedVector(ctx, N).upload2(dh)
    e = ctx.vector(N + 3, np.full(N + 3, POISON))
    Dy = ctx.vector(N, Dyh)
    ctx.check(ctx.L.lfpsqp_ineq_rhs(ctx.h, d.h, Dx.h, Dy.h, e.h))
    got = e.download()
    Dyi = i64(Dyh)
    assert np.array_equal(got[:N], np.abs(Dyi) * i64(dh)[:N] - i64(Dxh) * np.sign(Dyi) * i64(dh)[N:])
    assert np.array_equal(bits(got[N:]), bits(np.full(3, POISON)))
