"""Iteration time of projcg! with a GRID-STENCIL Hessian (a diagonal plus up to four off-diagonals at arbitrary distances) at n = 1e7, m = 128
(one MI355X): the fused ONE-pass iteration (lfpsqp_projcg_diags: DiagsMulF + DiagsGatherF / DiagsPrepSF + PcgFuseTri) against the callback path
with the same operator on the same buffers (lfpsqp_projcg_op: two passes over the basis per iteration).  The operator is kappa L + a for the
5-point (2-D grid), 7-point (3-D grid) or 9-point (2-D grid, --nine) stencil in row-major order.  --bounds: a stacked basis with four-way bounds
(none / lower / upper / both), as tools/time_band.py; --factored: the plain basis in factored form U = J W.  The set-up of the reduced operator
U'AU (once per solve: one shifted Gram pass per off-diagonal, plus one) is separated from the iterations by timing two solve lengths; the
break-even count is the set-up difference over the gain per iteration.
    python tools/time_diags.py [grid, e.g. 3200x3125 or 250x200x200] [m] [--nine] [--bounds] [--factored] [--json out.json] [--lib path]"""
import json, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import lfpsqp_jl_amd as L

out_json = lib = None
if "--lib" in sys.argv:
    k = sys.argv.index("--lib"); lib = L.load_library(sys.argv[k + 1]); del sys.argv[k:k + 2]
if "--json" in sys.argv:
    k = sys.argv.index("--json"); out_json = sys.argv[k + 1]; del sys.argv[k:k + 2]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
shape = tuple(int(s) for s in (args[0] if len(args) > 0 else "3200x3125").split("x"))
m = int(args[1]) if len(args) > 1 else 128
nine, bounds, factored = "--nine" in sys.argv, "--bounds" in sys.argv, "--factored" in sys.argv
assert not (bounds and factored), "--bounds times the materialised stacked basis"
assert not nine or len(shape) == 2, "--nine: a 2-D grid"
n = int(np.prod(shape))
ctx = L.Context(0, lib)
i = np.arange(n)
kappa = 0.9
if nine:                                   # edges -kappa, diagonals -kappa / 2
    ny, nx = shape
    r, c = np.divmod(i, nx)
    dists = (1, nx - 1, nx, nx + 1)
    offs = np.empty((n, 4), order="F")
    offs[:, 0] = np.where(c < nx - 1, -kappa, 0.0)
    offs[:, 1] = np.where((c > 0) & (r < ny - 1), -0.5 * kappa, 0.0)
    offs[:, 2] = np.where(r < ny - 1, -kappa, 0.0)
    offs[:, 3] = np.where((c < nx - 1) & (r < ny - 1), -0.5 * kappa, 0.0)
    deg = np.zeros(n)
    for k, s in enumerate(dists):
        deg[:n - s] -= offs[:n - s, k]
        deg[s:] -= offs[:n - s, k]
    del r, c
else:
    deg, offs, dists = L.grid_laplacian(shape, kappa)
off = ctx.matrix(n, len(dists), offs)
del offs
ax = deg + 0.05 + 0.5 * (0.5 + 0.5 * np.sin(0.37 * i)) ** 2          # kappa L + a, a in 0.05 .. 0.55
del deg
if bounds:
    from lfpsqp_jl_amd.inequality import InequalityData, InequalityDecomp, InequalityDecompProject, StackedVector, generate_initial_y_, inequality_gradient_
    xl = np.where((i % 4 == 1) | (i % 4 == 3), -1.0, -np.inf)
    xu = np.where((i % 4 == 2) | (i % 4 == 3), 1.0, np.inf)
    idata = InequalityData(ctx, xl, xu)
    xa = StackedVector(ctx, n)
    xa.upload(0.6 * np.sin(0.001 * i), 0)
    generate_initial_y_(xa, idata)
    Jct = ctx.matrix(n, m).hash_fill(1, 0, n, 1.0)
    dec = InequalityDecomp(ctx, n, m, Jct)
    inequality_gradient_(dec, xa, idata)
    S, Vt, rank = L.ksvd_(Jct, dec.Z, w2=dec.sx)
    dec.rank = rank
    U = InequalityDecompProject(dec)
    dg = StackedVector(ctx, n).upload2(np.concatenate([ax, np.full(n, 4.0)]))
    b = StackedVector(ctx, n)
    b.upload2(np.cos(0.002 * np.arange(2 * n)))
    x = StackedVector(ctx, n)
    work = L.ProjCGWork(ctx, 0, m, stacked_N=n)
elif factored:
    J = ctx.matrix(n, m, placed=True).hash_fill(1)
    W = np.zeros((m, m), order="F")
    S, Vt, rank = L.ksvd_(J, None, W=W)
    U = L.DeviceBasis(None, rank, generator=(J, W))
    work = L.ProjCGWork(ctx, n, m, against=J, extra=1)
    dg = work.placed_extra[0].upload(ax)
else:
    Z = ctx.matrix(n, m, placed=True).hash_fill(1)
    L.orthonormalize_(Z)
    U = L.DeviceBasis(Z)
    rank = m
    work = L.ProjCGWork(ctx, n, m, against=Z, extra=1)
    dg = work.placed_extra[0].upload(ax)
if not bounds:
    b = ctx.vector(n).hash_fill(4)
    x = ctx.vector(n)
del ax, i


def run(A, iters):
    best = 1e9
    for rep in range(3):
        ctx.sync(); t0 = time.perf_counter()
        it, nr = L.projcg_(x, None, A, U, b, None, tol=0.0, maxit=iters, work=work, want_lambda=False)
        ctx.sync(); best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, it, nr


def per_iteration(A):
    t1, i1, _ = run(A, 10)                 # (both lengths end before the residual reaches rounding level: no early exit)
    t2, i2, nr = run(A, 40)
    per = (t2 - t1) / (i2 - i1)
    return per, t1 - per * i1, nr, (i1, i2)


A = L.DiagonalsOperator(0.0, dg, off, dists)
p1, s1, nr1, it1 = per_iteration(A)
ctx.set_profiling(True)                    # kernel times of one 40-iteration solve on the one-pass path
run(A, 40)
ms, cnt = ctx.profile_read()
ctx.set_profiling(False)
res = dict(n=n, m=m, grid=list(shape), stencil=9 if nine else 2 * len(shape) + 1, distances=list(dists), rank=int(rank),
           bounds="four-way" if bounds else "none", basis="factored" if factored else "materialised", device=ctx.device_name,
           one_pass_ms_per_iter=round(p1, 4), one_pass_setup_ms=round(s1, 3), iterations=list(it1), nr_one_pass=nr1,
           profile_ms_per_launch={str(k): round(ms[k] / cnt[k], 4) for k in range(len(cnt)) if cnt[k] > 0})
if not factored:                           # (the callback path needs a materialised basis)
    A.fused = False
    p2, s2, nr2, it2 = per_iteration(A)
    res.update(callback_ms_per_iter=round(p2, 4), callback_setup_ms=round(s2, 3), speedup=round(p2 / p1, 3), iterations_callback=list(it2),
               nr_callback=nr2, break_even_iterations=(round((s1 - s2) / (p2 - p1), 1) if p2 > p1 else None))
print(f"grid={'x'.join(map(str, shape))} stencil={res['stencil']} m={m} bounds={res['bounds']} basis={res['basis']}: one pass {p1:.3f} ms/it "
      f"(+{s1:.2f} ms per solve)"
      + (f"; callback path {p2:.3f} ms/it (+{s2:.2f} ms per solve); speed-up {p2 / p1:.2f}x; break-even {res['break_even_iterations']} iterations; "
         f"nr {nr1:.6e} / {nr2:.6e}" if not factored else ""))
print(json.dumps(res))
if out_json:
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
