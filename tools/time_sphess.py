"""Iteration and set-up time of projcg! with a SPARSE SYMMETRIC Hessian (lfpsqp_projcg_sparse: couplings by row indices, DiagsMulF / DiagsGatherF
over SpHessD + PcgFuseTri, edge_width + 1 or + 2 gathered Gram passes per solve) at n ~ 1e7, m = 128 on one MI355X, against
  - the callback path with the same operator on the same buffers (`fused = False`: lfpsqp_projcg_op around lfpsqp_sphess_mul, two passes over the
    basis per iteration, no set-up), and
  - where the graph fits the distance form (at most 13 distinct distances j - i), lfpsqp_projcg_stencil on the same edges and buffers.  This
    is the stencil entry of the SAME build: its kernels are the instantiations DiagsMulF<DiagsD<13>> ... of functors whose template parameter
    changed from the descriptor's capacity to its type when the sparse kind was added -- the same code under another mangled name -- so it
    stands in for the entry as it was before; tools/time_diags.py GRID M --corners at the commit before gives the figure of that build itself.
The operator is kappa L + a on
  - a grid graph in row-major numbering (GRID = e.g. 216x216x216; --corners: 8 / 26 neighbours, --periodic: every axis closes on itself), or
  - --mesh: a triangulated 2-D grid (edges right, down and down-right; 6 neighbours per point); --permute: its vertices renumbered by a fixed
    random permutation (no locality left: thousands of distances).
The set-up (once per solve) is separated from the iterations by timing two solve lengths, as tools/time_diags.py does; the break-even count is
the set-up difference over the gain per iteration; where the one-pass form is SLOWER per iteration it never pays, the line says so, and
`SparseOperator.fused = False` is the choice for such a graph.  The modes are timed in alternation, --rounds times (default 3): the figures are medians,
"spread" the largest (max - min) / median of a mode over the rounds.
    python tools/time_sphess.py [GRID] [m] [--corners] [--periodic] [--mesh] [--permute] [--rounds R] [--json out.json] [--lib path]"""
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
shape = tuple(int(s) for s in (args[0] if len(args) > 0 else "216x216x216").split("x"))
m = int(args[1]) if len(args) > 1 else 128
periodic, corners, mesh, permute = (f in sys.argv for f in ("--periodic", "--corners", "--mesh", "--permute"))
assert not mesh or (len(shape) == 2 and not (periodic or corners)), "--mesh: a 2-D grid with the edges right, down and down-right"
n = int(np.prod(shape))
kappa = 0.9
t0 = time.perf_counter()
if mesh:
    ny, nx = shape
    v = np.arange(n)
    r, c = np.divmod(v, nx)
    ei = np.concatenate([v[c < nx - 1], v[r < ny - 1], v[(c < nx - 1) & (r < ny - 1)]])
    ej = np.concatenate([v[c < nx - 1] + 1, v[r < ny - 1] + nx, v[(c < nx - 1) & (r < ny - 1)] + nx + 1])
    del v, r, c
else:
    ei, ej = L.grid_edges(shape, periodic=periodic, corners=corners)
if permute:
    perm = np.random.default_rng(0).permutation(n)
    ei, ej = perm[ei], perm[ej]
    ei, ej = np.minimum(ei, ej), np.maximum(ei, ej)
    del perm
t_edges = time.perf_counter() - t0
ndist = int(np.count_nonzero(np.bincount(ej - ei)))
ctx = L.Context(0, lib)
t0 = time.perf_counter()
S = L.SparseHessian(ctx, n, ei, ej, -kappa)
t_create = time.perf_counter() - t0
deg = kappa * (np.bincount(ei, minlength=n) + np.bincount(ej, minlength=n))
ax = deg + 0.05 + 0.5 * (0.5 + 0.5 * np.sin(0.37 * np.arange(n))) ** 2          # kappa L + a, a in 0.05 .. 0.55
off = dists = None
if ndist <= 13:
    _, offs, dists = L.graph_diagonals(n, ei, ej, kappa)
    off = ctx.matrix(n, len(dists), offs)
    del offs
del ei, ej, deg
Z = ctx.matrix(n, m, placed=True).hash_fill(1)
L.orthonormalize_(Z)
U = L.DeviceBasis(Z)
work = L.ProjCGWork(ctx, n, m, against=Z, extra=1)
dg = work.placed_extra[0].upload(ax)
del ax
b = ctx.vector(n).hash_fill(4)
x = ctx.vector(n)


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


A = L.SparseOperator(0.0, dg, S)
Acb = L.SparseOperator(0.0, dg, S)
Acb.fused = False
modes = [("sparse_one_pass", A), ("sparse_callback", Acb)]
if off is not None:
    modes.append(("stencil_one_pass", L.DiagonalsOperator(0.0, dg, off, dists)))
meas = {name: [] for name, _ in modes}
for rnd in range(rounds):                  # the modes in alternation
    for name, op in modes:
        meas[name].append(per_iteration(op))
med = {name: (float(np.median([r[0] for r in rs])), float(np.median([r[1] for r in rs]))) for name, rs in meas.items()}
spread = max((max(r[0] for r in rs) - min(r[0] for r in rs)) / med[name][0] for name, rs in meas.items())
p1, s1 = med["sparse_one_pass"]
ctx.set_profiling(True)                    # kernel times of one 40-iteration solve on the one-pass path
run(A, 40)
ms, cnt = ctx.profile_read()
ctx.set_profiling(False)
graph = ("mesh" if mesh else "grid") + (" permuted" if permute else "") + (" periodic" if periodic else "") + (" corners" if corners else "")
res = dict(n=n, m=m, grid=list(shape), graph=graph, edges=S.nedges, distances=ndist, row_width=S.row_width, edge_width=S.edge_width,
           device=ctx.device_name, rounds=rounds, edge_list_s=round(t_edges, 2), create_s=round(t_create, 2),
           per_iter_ms={name: round(v[0], 4) for name, v in med.items()}, setup_ms={name: round(v[1], 3) for name, v in med.items()},
           per_iter_ms_by_round={name: [round(r[0], 4) for r in rs] for name, rs in meas.items()},
           setup_ms_by_round={name: [round(r[1], 3) for r in rs] for name, rs in meas.items()}, spread=round(spread, 4),
           nr={name: rs[0][2] for name, rs in meas.items()}, iterations=list(meas["sparse_one_pass"][0][3]),
           profile_ms_per_launch={str(k): round(ms[k] / cnt[k], 4) for k in range(len(cnt)) if cnt[k] > 0})
line = (f"{graph} {'x'.join(map(str, shape))} n={n} m={m} edges={S.nedges} distances={ndist} Kr={S.row_width} Ke={S.edge_width} "
        f"(create {t_create:.1f} s): sparse one pass {p1:.3f} ms/it (+{s1:.2f} ms per solve)")
for name in ("sparse_callback", "stencil_one_pass"):
    if name in med:
        p2, s2 = med[name]
        even = round((s1 - s2) / (p2 - p1), 1) if p2 > p1 else None
        res["break_even_iterations_vs_" + name] = even
        pays = f"break-even {even} iterations" if even is not None else "sparse one pass NEVER PAYS against it (slower per iteration)"
        line += f"; {name.replace('_', ' ')} {p2:.3f} ms/it (+{s2:.2f} ms per solve), ratio {p2 / p1:.2f}x, {pays}"
print(line + f"; spread over {rounds} rounds {100 * spread:.1f} %")
print(json.dumps(res))
if out_json:
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
