"""Time of lfpsqp_sphess_set_values (caller-supplied triplet values placed into both ELL forms of a handle and into the Hessian diagonal) on the
graphs of tools/time_sphess.py on one MI355X, on the SAME handle and in the same process next to
  - lfpsqp_sphess_mul (the yardstick: a streaming kernel of the same access class),
  - lfpsqp_sphess_edge_eval kind 0 with diag and H (the other producer of values),
  - a host rebuild (SparseHessian(...): lfpsqp_sphess_create, once) and the map's own build (lfpsqp_sphess_map_create, once).
The pattern: every edge once plus one diagonal triplet per row (no duplicates); --dups adds a second triplet for every fourth edge and a second
diagonal triplet for every fourth row, which switches the kernels to their chain-walking instantiation.  The modes alternate, --rounds times
(default 3), ten calls per measurement; medians, "spread" the largest (max - min) / median.  Algorithmic bytes:
    lfpsqp_sphess_mul        12 Kr + 24 per row                  (index 4 + value 8 per slot; v, dg, out)
    set_values               20 (Kr + Ke) + 20 per row           (position 4 + gathered value 8 + store 8 per slot of either form; the same for the diagonal)
    edge_eval kind 0, diag+H 28 (Kr + Ke) + 32 per row           (index 4 + weight 8 + gathered x 8 + store 8 per slot; x twice, diag read and written)
--outer [K]: the steady outer iteration of `optimize` (K and 2 K iterations, default 2; the difference over K) on ONE problem -- the objective,
gradient and linear equalities of GraphSeparableLinear on the device -- with its Lagrangian Hessian supplied three ways: through the pattern
interface (host values_, one upload and one lfpsqp_sphess_set_values per outer iteration, the solve on lfpsqp_projcg_sparse), through a host
hess_lag_vec_ callback (what `optimize` with host derivatives did before: one n-vector down and one up per CG iteration and the product on the
host), and by the device-resident class itself (the floor).  Every truncated-Newton solve runs exactly --tn iterations (default 5), no stopping
test of the outer loop is active and the line search is off, as in tools/time_sphess_edge.py.  One untimed run per way comes first.
    python tools/time_sphess_values.py [GRID] [m] [--corners] [--periodic] [--mesh] [--permute] [--dups] [--rounds R] [--outer [K]] [--tn T]
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
tn_fixed = opt("--tn", 5, int)
outer = None
if "--outer" in sys.argv:
    k = sys.argv.index("--outer")
    outer = int(sys.argv[k + 1]) if k + 1 < len(sys.argv) and sys.argv[k + 1].isdigit() else 2
    del sys.argv[k:k + (2 if k + 1 < len(sys.argv) and sys.argv[k + 1].isdigit() else 1)]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
shape = tuple(int(s) for s in (args[0] if len(args) > 0 else "3200x3125").split("x"))
m = int(args[1]) if len(args) > 1 else 128
periodic, corners, mesh, permute, dups = (f in sys.argv for f in ("--periodic", "--corners", "--mesh", "--permute", "--dups"))
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
res = dict(n=n, m=m, grid=list(shape), graph=graph, dups=bool(dups), device=ctx.device_name, rounds=rounds)
ar = np.arange(n)


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
    rows = [ei, ar] + ([ej[::4], ar[::4]] if dups else [])
    cols = [ej, ar] + ([ei[::4], ar[::4]] if dups else [])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    t0 = time.perf_counter()
    pat = L.SparsePattern(W, rows, cols)
    t_map = time.perf_counter() - t0
    del ei, ej, rows, cols
    H = W.like()
    x = ctx.vector(n).hash_fill(2, scale=2.4, shift=-1.2)
    vals = ctx.vector(pat.nnz).hash_fill(3)
    d, out = ctx.vector(n), ctx.vector(n)
    A = L.SparseOperator(0.0, d, H)
    modes = [("sphess_mul", lambda: A.mul_(out, x)),
             ("set_values", lambda: pat.set_values(vals, diag=d, out=H)),
             ("set_values_H_only", lambda: pat.set_values(vals, out=H)),
             ("edge_eval_kind0_diag_H", lambda: W.edge_eval(0, 0.0, kappa, x, None, d, H, want_f=False))]
    meas = {name: [] for name, _ in modes}
    for rnd in range(rounds):
        for name, fn in modes:
            meas[name].append(timed(fn))
    med = {name: float(np.median(v)) for name, v in meas.items()}
    spread = max((max(v) - min(v)) / med[name] for name, v in meas.items())
    kr, ke = W.row_width, W.edge_width
    gbytes = dict(sphess_mul=(12.0 * kr + 24.0) * n / 1e9, set_values=(20.0 * (kr + ke) + 20.0) * n / 1e9,
                  set_values_H_only=20.0 * (kr + ke) * n / 1e9, edge_eval_kind0_diag_H=(28.0 * (kr + ke) + 32.0) * n / 1e9)
    res.update(edges=W.nedges, row_width=kr, edge_width=ke, nnz=pat.nnz, max_dup=pat.max_dup, create_s=round(t_create, 2), map_create_s=round(t_map, 2),
               ms={k: round(v, 4) for k, v in med.items()}, ms_by_round={k: [round(t, 4) for t in v] for k, v in meas.items()},
               spread=round(spread, 4), algorithmic_gb={k: round(v, 3) for k, v in gbytes.items()},
               tb_per_s={k: round(gbytes[k] / med[k], 3) for k in med},
               time_ratio_to_mul={k: round(med[k] / med["sphess_mul"], 3) for k in med},
               byte_ratio_to_mul={k: round(gbytes[k] / gbytes["sphess_mul"], 3) for k in med})
    print(f"{graph} {'x'.join(map(str, shape))} n={n} edges={W.nedges} Kr={kr} Ke={ke} nnz={pat.nnz} max_dup={pat.max_dup} (handle {t_create:.1f} s, "
          f"map {t_map:.1f} s on the host): " +
          "; ".join(f"{k.replace('_', ' ')} {med[k]:.3f} ms ({gbytes[k] / med[k]:.2f} TB/s of {gbytes[k]:.2f} GB, x{med[k] / med['sphess_mul']:.2f} "
                    f"time for x{gbytes[k] / gbytes['sphess_mul']:.2f} bytes)" for k in med) + f"; spread over {rounds} rounds {100 * spread:.1f} %")
else:
    from lfpsqp_jl_amd.optimize import optimize_core
    from lfpsqp_jl_amd.problems import _SparsePatternHessian
    Jct = ctx.matrix(n, m, placed=True).hash_fill(1)
    xs = ctx.vector(n).hash_fill(2)
    b = ctx.vector(m); L.gemv_t(Jct, xs, b)
    bh = b.download()
    a = 0.5 + np.linspace(0.0, 1.0, n) ** 2
    x0 = np.cos(np.arange(n) * 1e-3)
    P = L.GraphSeparableLinear(ctx, n, m, Jct, bh, 1, a, 0.0, edges=(ei, ej, 1.0), kappa=kappa)      # phi = a t^4 + t^2: phi'' = 12 a t^2 + 2
    deg = kappa * (np.bincount(ei, minlength=n) + np.bincount(ej, minlength=n)).astype(np.float64)
    calls = dict(values=0, hlv=0)

    def values_(vals, x, lam):                             # the edges -kappa, the diagonal phi''(x) + kappa deg
        calls["values"] += 1
        vals[:len(ei)] = -kappa
        np.multiply(x, x, out=vals[len(ei):])
        vals[len(ei):] *= 12.0 * a
        vals[len(ei):] += 2.0 + deg

    def hlv_dev(dest, src, x, lam):                        # the host callback of problems._host_core: two n-vectors down, one up, the product on the host
        calls["hlv"] += 1
        s, xh = src.download(n, 0), x.download(n, 0)
        o = (12.0 * a * xh * xh + 2.0 + deg) * s
        o -= kappa * (np.bincount(ei, s[ej], n) + np.bincount(ej, s[ei], n))
        dest.upload(o, 0)

    t0 = time.perf_counter()
    hess = _SparsePatternHessian(ctx, n, n, L.SparseLagrangianHessian(np.concatenate([ei, ar]), np.concatenate([ej, ar]), values_))
    t_setup = time.perf_counter() - t0

    def run(h, k, trace=None):
        ctx.sync(); t0 = time.perf_counter()
        par = L.LFPSQPParams(do_project_retract=False, disp=L.DisplayOption.off, maxiter=k, tn_kappa=0.0, tn_maxiter=tn_fixed, eps_f=0.0, eps_x=0.0,
                             eps_kkt=0.0, disable_linesearch=True)
        x, obj, lam, ti = optimize_core(P.f, P.grad_, P.cons, P.jac_, h, x0, None, None, m, par, ctx=ctx, trace=trace)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, ti.iter, obj[-1]

    ways = [("pattern", hess), ("host_callback", hlv_dev), ("device_class", P)]
    meas = {name: [] for name, _ in ways}
    fin = {}
    for name, h in ways:                                   # (first allocations, placement probes)
        fin[name] = float(run(h, outer)[2])
    for rnd in range(rounds):
        for name, h in ways:
            t1, i1, _ = run(h, outer)
            t2, i2, _ = run(h, 2 * outer)
            meas[name].append((t2 - t1) / max(i2 - i1, 1))
    med = {name: float(np.median(v)) for name, v in meas.items()}
    spread = max((max(v) - min(v)) / med[name] for name, v in meas.items())
    S = hess.sparse_hessian
    res.update(edges=S.nedges, row_width=S.row_width, edge_width=S.edge_width, outer_iterations=[outer, 2 * outer], tn_fixed=tn_fixed,
               outer_ms={k: round(v, 3) for k, v in med.items()}, outer_ms_by_round={k: [round(t, 3) for t in v] for k, v in meas.items()},
               spread=round(spread, 4), pattern_setup_s=round(t_setup, 2), calls=calls, objective_after_first_run=fin)
    print(f"{graph} {'x'.join(map(str, shape))} n={n} m={m}: outer iteration with {tn_fixed} CG iterations per solve: pattern interface "
          f"{med['pattern']:.2f} ms, host hess_lag_vec_ callback {med['host_callback']:.2f} ms, device-resident class {med['device_class']:.2f} ms; "
          f"handle and map built once in {t_setup:.1f} s; objective after {outer} iterations {fin}; spread over {rounds} rounds {100 * spread:.1f} %")
print(json.dumps(res))
if out_json:
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
