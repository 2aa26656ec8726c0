"""Iteration time of projcg! with a GRID-STENCIL Hessian (a diagonal plus up to 13 off-diagonals at arbitrary distances) at n = 1e7, m = 128
(one MI355X): the fused ONE-pass iteration (lfpsqp_projcg_diags / lfpsqp_projcg_stencil: DiagsMulF + DiagsGatherF / DiagsPrepSF + PcgFuseTri)
against the callback path with the same operator on the same buffers (lfpsqp_projcg_op: two passes over the basis per iteration).  The operator
is kappa L + a for the 5-point (2-D grid), 7-point (3-D grid) or 9-point (2-D grid, --nine) stencil in row-major order; --corners: every point
coupled to its 8 / 26 neighbours with weight kappa (4 / 13 off-diagonals); --periodic: every axis closes on itself (4 / 6 off-diagonals, 10
with --corners in 2-D).  --bounds: a stacked basis with four-way bounds (none / lower / upper / both), as tools/time_band.py; --factored: the
plain basis in factored form U = J W.  --split-callback: the callback path also with the SAME Hessian as a sum of DiagonalsOperators of at most
four off-diagonals each behind one Python mul_ (all that was possible while one operator held four: several product launches per
iteration).  The set-up of the reduced operator U'AU (once per solve: one shifted Gram pass per off-diagonal, plus one or two) is separated from
the iterations by timing two solve lengths; the break-even count is the set-up difference over the gain per iteration.  The modes are timed
in alternation, --rounds times (default 3): the figures are medians, "spread" the largest (max - min) / median of a mode over the rounds.
    python tools/time_diags.py [grid, e.g. 3200x3125 or 250x200x200] [m] [--nine] [--corners] [--periodic] [--bounds] [--factored]
                               [--split-callback] [--rounds R] [--json out.json] [--lib path]"""
import json, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import lfpsqp_jl_amd as L

out_json = lib = None
if "--lib" in sys.argv:
    k = sys.argv.index("--lib"); lib = L.load_library(sys.argv[k + 1]); del sys.argv[k:k + 2]
if "--json" in sys.argv:
    k = sys.argv.index("--json"); out_json = sys.argv[k + 1]; del sys.argv[k:k + 2]
rounds = 3
if "--rounds" in sys.argv:
    k = sys.argv.index("--rounds"); rounds = int(sys.argv[k + 1]); del sys.argv[k:k + 2]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
shape = tuple(int(s) for s in (args[0] if len(args) > 0 else "3200x3125").split("x"))
m = int(args[1]) if len(args) > 1 else 128
nine, bounds, factored = "--nine" in sys.argv, "--bounds" in sys.argv, "--factored" in sys.argv
assert not (bounds and factored), "--bounds times the materialised stacked basis"
assert not nine or len(shape) == 2, "--nine: a 2-D grid"
periodic, corners, split = "--periodic" in sys.argv, "--corners" in sys.argv, "--split-callback" in sys.argv
assert not (nine and (periodic or corners)), "--nine is the weighted 9-point stencil of its own"
assert not (split and factored), "the callback path needs a materialised basis"
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
    deg, offs, dists = L.grid_laplacian(shape, kappa, periodic=periodic, corners=corners)
off = ctx.matrix(n, len(dists), offs)
off_split = [ctx.matrix(n, len(dists[k:k + 4]), np.asfortranarray(offs[:, k:k + 4])) for k in range(0, len(dists), 4)] if split else []
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


class SplitOperator:
    """The same A as a sum of operators of at most four off-diagonals each (the diagonal with the first), behind one mul_."""

    def __init__(self):
        self.parts = [L.DiagonalsOperator(0.0, dg if k == 0 else None, o, dists[4 * k:4 * k + 4]) for k, o in enumerate(off_split)]

    def mul_(self, dest, v):
        self.parts[0].mul_(dest, v)
        for p in self.parts[1:]:
            p.mul_(dest, v, 1.0, 1.0)
        return dest

    def adjoint(self):
        return self


A = L.DiagonalsOperator(0.0, dg, off, dists)
Acb = L.DiagonalsOperator(0.0, dg, off, dists)
Acb.fused = False
modes = [("one_pass", A)] + ([] if factored else [("callback", Acb)]) + ([("split_callback", SplitOperator())] if split else [])
meas = {name: [] for name, _ in modes}
for rnd in range(rounds):                  # the modes in alternation
    for name, op in modes:
        meas[name].append(per_iteration(op))
med = {name: (float(np.median([r[0] for r in rs])), float(np.median([r[1] for r in rs]))) for name, rs in meas.items()}
spread = max((max(r[0] for r in rs) - min(r[0] for r in rs)) / med[name][0] for name, rs in meas.items())
p1, s1 = med["one_pass"]
nr1, it1 = meas["one_pass"][0][2], meas["one_pass"][0][3]
ctx.set_profiling(True)                    # kernel times of one 40-iteration solve on the one-pass path
run(A, 40)
ms, cnt = ctx.profile_read()
ctx.set_profiling(False)
stencil = 9 if nine else (3 ** len(shape) if corners else 2 * len(shape) + 1)
res = dict(n=n, m=m, grid=list(shape), stencil=stencil, periodic=periodic, distances=list(dists), rank=int(rank),
           bounds="four-way" if bounds else "none", basis="factored" if factored else "materialised", device=ctx.device_name, rounds=rounds,
           one_pass_ms_per_iter=round(p1, 4), one_pass_setup_ms=round(s1, 3), iterations=list(it1), nr_one_pass=nr1,
           per_iter_ms_by_round={name: [round(r[0], 4) for r in rs] for name, rs in meas.items()},
           setup_ms_by_round={name: [round(r[1], 3) for r in rs] for name, rs in meas.items()}, spread=round(spread, 4),
           profile_ms_per_launch={str(k): round(ms[k] / cnt[k], 4) for k in range(len(cnt)) if cnt[k] > 0})
line = (f"grid={'x'.join(map(str, shape))} stencil={stencil}{' periodic' if periodic else ''} K={len(dists)} m={m} bounds={res['bounds']} "
        f"basis={res['basis']}: one pass {p1:.3f} ms/it (+{s1:.2f} ms per solve)")
for name in ("callback", "split_callback"):
    if name in med:
        p2, s2 = med[name]
        res.update({name + "_ms_per_iter": round(p2, 4), name + "_setup_ms": round(s2, 3), "speedup_over_" + name: round(p2 / p1, 3),
                    "iterations_" + name: list(meas[name][0][3]), "nr_" + name: meas[name][0][2],
                    "break_even_iterations_" + name: (round((s1 - s2) / (p2 - p1), 1) if p2 > p1 else None)})
        line += (f"; {name.replace('_', ' ')} {p2:.3f} ms/it (+{s2:.2f} ms per solve), speed-up {p2 / p1:.2f}x, break-even "
                 f"{res['break_even_iterations_' + name]} iterations, nr {meas[name][0][2]:.6e}")
print(line + f"; nr one pass {nr1:.6e}; spread over {rounds} rounds {100 * spread:.1f} %")
print(json.dumps(res))
if out_json:
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
