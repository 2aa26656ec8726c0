"""Time of lfpsqp_sphess_edge_eval (a non-quadratic edge term on a graph: value, gradient, diagonal and the refreshed Hessian values in both ELL
forms) on the graphs of tools/time_sphess.py at n ~ 1e7 on one MI355X, next to lfpsqp_sphess_mul on the SAME handle in the same process:
  - the full call (f, grad, diag, H), the call without f (no reduction), and the value-only call (what a line search pays per trial);
  - the modes alternate, --rounds times (default 3), ten calls per measurement; the figures are medians, "spread" the largest (max - min) / median.
Algorithmic bytes per stored row entry (a row's slot: int32 index + fp64 value), gathers of x counted as 8:
    lfpsqp_sphess_mul        4 + 8 + 8                      = 20      (+ 24 per row: v, dg, out)
    value only               4 + 8 + 8                      = 20      (+ 8 per row: x)
    full                     4 + 8 + 8 + 8 (store) + (4 + 8 + 8 + 8) Ke / Kr for the edge form   (+ 40 per row: x, grad and diag read and written;
                             the edge launch reads x again: + 8)
--outer [K]: the steady outer iteration of `optimize` (K and 2 K iterations, default 4; the difference over K) for GraphPotentialLinear against
GraphSeparableLinear on the same graph, constraints and separable part -- the constant-Hessian floor -- and lfpsqp_sphess_create timed once: the
only route to new values before lfpsqp_sphess_edge_eval.  So that both classes do the same work per outer iteration, every truncated-Newton solve
runs exactly --tn iterations (default 10: tolerance 0), no stopping test of the outer loop is active and the line search is off (full steps: with
it, the number of trial retractions -- different objectives, different trajectories -- decides the time).  One untimed run per class comes first.
    python tools/time_sphess_edge.py [GRID] [m] [--corners] [--periodic] [--mesh] [--permute] [--kind K] [--delta D] [--rounds R] [--outer [K]] [--tn T]
                                     [--json out.json] [--lib path]"""
import json, os, sys, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import lfpsqp_jl_amd as L


def opt(name, default, conv):
    if name not in sys.argv:
        return default
    k = sys.argv.index(name)
    v = conv(sys.argv[k + 1])
    del sys.argv[k:k + 2]
    return v


lib = opt("--lib", None, L.load_library)
out_json = opt("--json", None, str)
rounds = opt("--rounds", 3, int)
kind = opt("--kind", 2, int)
delta = opt("--delta", 0.5, float)
tn_fixed = opt("--tn", 10, int)
outer = None
if "--outer" in sys.argv:
    k = sys.argv.index("--outer")
    outer = int(sys.argv[k + 1]) if k + 1 < len(sys.argv) and sys.argv[k + 1].isdigit() else 4
    del sys.argv[k:k + (2 if k + 1 < len(sys.argv) and sys.argv[k + 1].isdigit() else 1)]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
shape = tuple(int(s) for s in (args[0] if len(args) > 0 else "3200x3125").split("x"))
m = int(args[1]) if len(args) > 1 else 128
periodic, corners, mesh, permute = (f in sys.argv for f in ("--periodic", "--corners", "--mesh", "--permute"))
assert not mesh or (len(shape) == 2 and not (periodic or corners)), "--mesh: a 2-D grid with the edges right, down and down-right"
n = int(np.prod(shape))
kappa = 0.9
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
ctx = L.Context(0, lib)
graph = ("mesh" if mesh else "grid") + (" permuted" if permute else "") + (" periodic" if periodic else "") + (" corners" if corners else "")
res = dict(n=n, m=m, grid=list(shape), graph=graph, kind=kind, delta=delta, device=ctx.device_name, rounds=rounds)


def timed(fn, reps=10):
    fn()
    ctx.sync(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


if outer is None:
    t0 = time.perf_counter()
    W = L.SparseHessian(ctx, n, ei, ej, 1.0)
    t_create = time.perf_counter() - t0
    del ei, ej
    H = W.like()
    x = ctx.vector(n).hash_fill(2, scale=2.4, shift=-1.2)
    g, d, out = ctx.vector(n), ctx.vector(n), ctx.vector(n)
    A = L.SparseOperator(0.0, d, H)
    modes = [("sphess_mul", lambda: A.mul_(out, x)),
             ("edge_eval_full", lambda: W.edge_eval(kind, delta, kappa, x, g, d, H)),
             ("edge_eval_no_f", lambda: W.edge_eval(kind, delta, kappa, x, g, d, H, want_f=False)),
             ("edge_eval_diag_H", lambda: W.edge_eval(kind, delta, kappa, x, None, d, H, want_f=False)),
             ("edge_eval_f_only", lambda: W.edge_eval(kind, delta, kappa, x))]
    meas = {name: [] for name, _ in modes}
    for rnd in range(rounds):
        for name, fn in modes:
            meas[name].append(timed(fn))
    med = {name: float(np.median(v)) for name, v in meas.items()}
    spread = max((max(v) - min(v)) / med[name] for name, v in meas.items())
    kr, ke = W.row_width, W.edge_width
    per_entry = dict(sphess_mul=20.0, edge_eval_f_only=20.0, edge_eval_full=28.0 + 28.0 * ke / kr)
    per_row = dict(sphess_mul=24.0, edge_eval_f_only=8.0, edge_eval_full=48.0)
    gbytes = {k: (per_entry[k] * kr + per_row[k]) * n / 1e9 for k in per_entry}
    gbytes["edge_eval_no_f"] = gbytes["edge_eval_full"]
    gbytes["edge_eval_diag_H"] = gbytes["edge_eval_full"] - 16.0 * n / 1e9           # (grad is neither read nor written)
    res.update(edges=W.nedges, row_width=kr, edge_width=ke, create_s=round(t_create, 2), ms={k: round(v, 4) for k, v in med.items()},
               ms_by_round={k: [round(t, 4) for t in v] for k, v in meas.items()}, spread=round(spread, 4),
               bytes_per_entry=per_entry, algorithmic_gb={k: round(v, 3) for k, v in gbytes.items()},
               tb_per_s={k: round(gbytes[k] / med[k], 3) for k in med},
               time_ratio_to_mul={k: round(med[k] / med["sphess_mul"], 3) for k in med},
               byte_ratio_to_mul={k: round(gbytes[k] / gbytes["sphess_mul"], 3) for k in med})
    print(f"{graph} {'x'.join(map(str, shape))} n={n} edges={W.nedges} Kr={kr} Ke={ke} kind={kind} (create {t_create:.1f} s): " +
          "; ".join(f"{k.replace('_', ' ')} {med[k]:.3f} ms ({gbytes[k] / med[k]:.2f} TB/s of {gbytes[k]:.2f} GB, x{med[k] / med['sphess_mul']:.2f} "
                    f"time for x{gbytes[k] / gbytes['sphess_mul']:.2f} bytes)" for k in med) + f"; spread over {rounds} rounds {100 * spread:.1f} %")
else:
    Jct = ctx.matrix(n, m, placed=True).hash_fill(1)
    xs = ctx.vector(n).hash_fill(2)
    b = ctx.vector(m); L.gemv_t(Jct, xs, b)
    bh = b.download()
    a = 0.5 + np.linspace(0.0, 1.0, n) ** 2
    x0 = np.cos(np.arange(n) * 1e-3)
    t0 = time.perf_counter()
    P = L.GraphPotentialLinear(ctx, n, m, Jct, bh, 1, a, 0.0, edges=(ei, ej, 1.0), kappa=kappa, edge_kind=kind, delta=delta)
    t_pot = time.perf_counter() - t0
    t0 = time.perf_counter()
    Q = L.GraphSeparableLinear(ctx, n, m, Jct, bh, 1, a, 0.0, edges=(ei, ej, 1.0), kappa=kappa)
    t_create = time.perf_counter() - t0                    # (one lfpsqp_sphess_create and a degree vector: the price of new values without edge_eval)
    del ei, ej

    def run(prob, k, trace=None):
        ctx.sync(); t0 = time.perf_counter()
        x, obj, lam, ti = prob.optimize(x0, L.LFPSQPParams(do_project_retract=False, disp=L.DisplayOption.off, maxiter=k, tn_kappa=0.0, tn_maxiter=tn_fixed,
                                                           eps_f=0.0, eps_x=0.0, eps_kkt=0.0, disable_linesearch=True), trace=trace)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, ti.iter

    probs = [("graph_potential", P), ("graph_separable", Q)]
    meas = {name: [] for name, _ in probs}
    for name, prob in probs:                               # (first allocations, placement probes)
        run(prob, outer)
    for rnd in range(rounds):
        for name, prob in probs:
            t1, i1 = run(prob, outer)
            t2, i2 = run(prob, 2 * outer)
            meas[name].append((t2 - t1) / max(i2 - i1, 1))
    tn, ls = {}, {}
    for name, prob in probs:                               # (a traced run for the counts: the trace downloads x, so it is not timed)
        tr = []
        run(prob, 2 * outer, tr)
        tn[name] = [t.get('tn_iter') or 0 for t in tr]
        ls[name] = [t.get('alpha') for t in tr]
    med = {name: float(np.median(v)) for name, v in meas.items()}
    spread = max((max(v) - min(v)) / med[name] for name, v in meas.items())
    res.update(edges=P.weights.nedges, row_width=P.weights.row_width, edge_width=P.weights.edge_width, outer_iterations=[outer, 2 * outer],
               outer_ms={k: round(v, 3) for k, v in med.items()}, outer_ms_by_round={k: [round(t, 3) for t in v] for k, v in meas.items()},
               tn_iterations=tn, tn_fixed=tn_fixed, accepted_alpha=ls, spread=round(spread, 4), handle_create_s=round(t_create, 2), potential_setup_s=round(t_pot, 2))
    print(f"{graph} {'x'.join(map(str, shape))} n={n} m={m} kind={kind}: outer iteration GraphPotentialLinear {med['graph_potential']:.2f} ms "
          f"(truncated-Newton iterations {tn['graph_potential']}), GraphSeparableLinear {med['graph_separable']:.2f} ms ({tn['graph_separable']}); "
          f"a handle rebuilt on the host {t_create:.1f} s; spread over {rounds} rounds {100 * spread:.1f} %")
print(json.dumps(res))
if out_json:
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
