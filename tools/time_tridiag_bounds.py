"""Iteration time of projcg! with a TRIDIAGONAL Hessian and BOUNDS at n = 1e7, m = 128 (one MI355X): the stacked one-pass iteration
(lfpsqp_projcg_tridiag over InequalityDecompProject: TriPrepSF + PcgFuseTri<true, .>) against the callback path with the same operator on the
same buffers (lfpsqp_projcg_op: two passes over Z per iteration), and the stacked diagonal operator alone.  Four-way bounds (none / lower /
upper / both).  The set-up of the reduced operator (once per solve) is separated from the iterations by timing two solve lengths.
    python tools/time_tridiag_bounds.py [n] [m] [--json out.json] [--lib path]"""
import json, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import lfpsqp_jl_amd as L
from lfpsqp_jl_amd.inequality import InequalityData, InequalityDecomp, InequalityDecompProject, StackedVector, generate_initial_y_, inequality_gradient_

out_json = lib = None
if "--lib" in sys.argv:
    k = sys.argv.index("--lib"); lib = L.load_library(sys.argv[k + 1]); del sys.argv[k:k + 2]
if "--json" in sys.argv:
    k = sys.argv.index("--json"); out_json = sys.argv[k + 1]; del sys.argv[k:k + 2]
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
m = int(sys.argv[2]) if len(sys.argv) > 2 else 128
ctx = L.Context(0, lib)
i = np.arange(n)
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
Q = InequalityDecompProject(dec)
dg = StackedVector(ctx, n).upload2(np.concatenate([2.0 + 9.0 * (0.5 + 0.5 * np.sin(0.37 * i)), np.full(n, 4.0)]))   # x half 2 .. 11, y half 4
off = ctx.vector(n).hash_fill(15, 0, 0.8, 0.0)                 # couplings of both signs, |off| <= 0.8 (x half)
b = StackedVector(ctx, n)
b.upload2(np.cos(0.002 * np.arange(2 * n)))
x = StackedVector(ctx, n)
work = L.ProjCGWork(ctx, 0, m, stacked_N=n)


def run(A, iters):
    best = 1e9
    for rep in range(3):
        ctx.sync(); t0 = time.perf_counter()
        it, nr = L.projcg_(x, None, A, Q, b, None, tol=0.0, maxit=iters, work=work, want_lambda=False)
        ctx.sync(); best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, it, nr


def per_iteration(A):
    t1, i1, _ = run(A, 10)                 # (both lengths end before the residual reaches rounding level: no early exit)
    t2, i2, nr = run(A, 40)
    per = (t2 - t1) / (i2 - i1)
    return per, t1 - per * i1, nr, (i1, i2)


p0, s0, nr0, _ = per_iteration(L.DiagOperator(0.0, dg))
A = L.TridiagonalOperator(0.0, dg, off)
p1, s1, nr1, it1 = per_iteration(A)
ctx.set_profiling(True)                    # kernel times of one 40-iteration solve on the one-pass path
run(A, 40)
ms, cnt = ctx.profile_read()
ctx.set_profiling(False)
A.fused = False
p2, s2, nr2, it2 = per_iteration(A)
res = dict(n=n, m=m, rank=int(rank), bounds="four-way", device=ctx.device_name,
           diagonal_ms_per_iter=round(p0, 4), one_pass_ms_per_iter=round(p1, 4), one_pass_setup_ms=round(s1, 3),
           callback_ms_per_iter=round(p2, 4), callback_setup_ms=round(s2, 3), speedup=round(p2 / p1, 3),
           iterations=list(it1), iterations_callback=list(it2), nr_one_pass=nr1, nr_callback=nr2,
           profile_ms_per_launch={str(k): round(ms[k] / cnt[k], 4) for k in range(len(cnt)) if cnt[k] > 0})
print(f"n={n} m={m} four-way bounds: diagonal {p0:.3f} ms/it; tridiagonal one pass {p1:.3f} ms/it (+{s1:.2f} ms per solve); "
      f"callback path {p2:.3f} ms/it; speed-up {p2 / p1:.2f}x; nr {nr1:.6e} / {nr2:.6e}")
print(json.dumps(res))
if out_json:
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
