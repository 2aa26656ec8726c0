"""Time of lfpsqp_sphess_pair_eval (a pair potential between points of 2 or 3 unknowns each: value, gradient, diagonal and the refreshed Hessian
values in both ELL forms) on a lattice of points built with grid_edges, on one MI355X, for each kind, next to the yardstick in the same process:
lfpsqp_sphess_edge_eval kind 2 with all outputs on the SAME handle -- a handle of points is an ordinary handle, so the scalar kernels run over the
identical pattern, row width and edge width (its values mean nothing there; the time does not depend on them).
  - the modes alternate, --rounds times (default 3), ten calls per measurement; the figures are medians, "spread" the largest (max - min) / median.
Algorithmic bytes per call, n scalar rows, the ELL widths Kr and Ke (every slot of an ELL array is read, stored or empty):
    streamed:   (4 + 8 read, 8 written) = 20 per slot of either form                      20 (Kr + Ke) n
    row vectors: x read by both launches, grad and diag read and written                   48 n
    gathers of x, counted as 8 each: pair: dim per neighbour and row in the row form (8 per slot), dim per slot in the edge form;
                scalar: one per slot of either form                                         8 (Kr + dim Ke) n   /   8 (Kr + Ke) n
The HBM peak is taken as 8 TB/s (6.3 TB/s is what a plain copy reaches).
    python tools/time_sphess_pair.py [GRID] [--delta D] [--rounds R] [--rest-per-edge] [--anchors K] [--json out.json] [--lib path]
GRID: 3200x3125 (dim 2, the default) or 150x150x150 (dim 3): the number of axes is dim.
--rest-per-edge and --anchors K (K anchors on every point, at most 8) add modes of lfpsqp_sphess_pair_eval_ex, kind 1 with all outputs, that
alternate with the uniform pair_eval on the SAME handle in the same rounds: "ex_rest" (a rest length per edge: 28 instead of 20 bytes per stored
slot of either form), "ex_anchors<K>" (24 K bytes per row more) and, with both options, "ex_rest_anchors<K>"; "ratio_to_uniform_kind1" is their
time over pair_eval kind 1, "byte_ratio" the same ratio of the streamed bytes."""
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
delta = opt("--delta", 0.8, float)
nanch = opt("--anchors", 0, int)
rest_per_edge = "--rest-per-edge" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
shape = tuple(int(s) for s in (args[0] if len(args) > 0 else "3200x3125").split("x"))
dim = len(shape)
assert dim in (2, 3), "GRID: two or three axes"
npoints = int(np.prod(shape))
n = dim * npoints
kappa = 0.9
HBM_PEAK_TBS = 8.0
pi, pj = L.grid_edges(shape)
ctx = L.Context(0, lib)
res = dict(n=n, npoints=npoints, dim=dim, grid=list(shape), delta=delta, device=ctx.device_name, rounds=rounds)


def timed(fn, reps=10):
    fn()
    ctx.sync(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


t0 = time.perf_counter()
W = L.SparseHessian.from_points(ctx, n, npoints, dim, pi, pj, 1.0)
t_create = time.perf_counter() - t0
# a rest length per edge, delta (1 +- 0.2)
P = W.point_values(pi, pj, delta * (1.0 + 0.2 * (2.0 * np.random.default_rng(1).random(len(pi)) - 1.0))) if rest_per_edge else None
del pi, pj
H = W.like()
# the points within 0.2 of their lattice places (spacing 1): r between 0.6 and 1.4 on every edge
xh = np.indices(shape).reshape(dim, -1).T.astype(np.float64) + 0.4 * (np.random.default_rng(0).random((npoints, dim)) - 0.5)
x = ctx.vector(n, xh.ravel())
A = None
if nanch > 0:       # K anchors on every point, 0.6 .. 1.4 away from it, with their own rest lengths
    rng = np.random.default_rng(2)
    off = rng.standard_normal((npoints, nanch, dim))
    off *= (0.6 + 0.8 * rng.random((npoints, nanch)) / np.sqrt(np.sum(off * off, axis=2)))[:, :, None]
    A = L.PointAnchors(W, np.repeat(np.arange(npoints, dtype=np.int64), nanch), (xh[:, None, :] + off).reshape(-1, dim), 1.0,
                       delta * (0.8 + 0.4 * rng.random(npoints * nanch)))
    del off
del xh
g, d = ctx.vector(n), ctx.vector(n)
modes = [("edge_eval_kind2", lambda: W.edge_eval(2, delta, kappa, x, g, d, H))] + \
        [(f"pair_eval_kind{k}", (lambda k: lambda: W.pair_eval(k, delta, kappa, x, g, d, H))(k)) for k in (0, 1, 2)] + \
        [("pair_eval_kind2_f_only", lambda: W.pair_eval(2, delta, kappa, x))]
ex = ([("ex_rest", P, None)] if P is not None else []) + ([(f"ex_anchors{nanch}", None, A)] if A is not None else []) + \
     ([(f"ex_rest_anchors{nanch}", P, A)] if P is not None and A is not None else [])
modes += [(name, (lambda p, a: lambda: W.pair_eval(1, delta, kappa, x, g, d, H, params=p, anchors=a))(p, a)) for name, p, a in ex]
meas = {name: [] for name, _ in modes}
for rnd in range(rounds):
    for name, fn in modes:
        meas[name].append(timed(fn))
med = {name: float(np.median(v)) for name, v in meas.items()}
spread = max((max(v) - min(v)) / med[name] for name, v in meas.items())
kr, ke = W.row_width, W.edge_width
slots = (kr + ke) * n
streamed = 20.0 * slots + 48.0 * n
gb = {name: (streamed + 8.0 * (kr + (dim if name.startswith(("pair", "ex")) else 1) * ke) * n) / 1e9 for name in med}
gb["pair_eval_kind2_f_only"] = (12.0 * kr * n + 8.0 * n + 8.0 * kr * n) / 1e9
# a parameter: 8 more per slot of either form; anchors: 24 per row and slot of width
bytes_ex = {name: streamed + (8.0 * slots if p is not None else 0.0) + (24.0 * nanch * n if a is not None else 0.0) for name, p, a in ex}
for name, v in bytes_ex.items():
    gb[name] += (v - streamed) / 1e9
res.update(scalar_edges=W.nedges, row_width=kr, edge_width=ke, create_s=round(t_create, 2), ms={k: round(v, 4) for k, v in med.items()},
           ms_by_round={k: [round(t, 4) for t in v] for k, v in meas.items()}, spread=round(spread, 4),
           algorithmic_gb={k: round(v, 3) for k, v in gb.items()}, streamed_gb=round(streamed / 1e9, 3),
           tb_per_s={k: round(gb[k] / med[k], 3) for k in med}, hbm_peak_fraction={k: round(gb[k] / med[k] / HBM_PEAK_TBS, 3) for k in med},
           ns_per_slot={k: round(med[k] * 1e6 / slots, 5) for k in med if not k.endswith("f_only")},
           time_ratio_to_scalar={k: round(med[k] / med["edge_eval_kind2"], 3) for k in med})
if ex:
    res.update(ratio_to_uniform_kind1={k: round(med[k] / med["pair_eval_kind1"], 4) for k in bytes_ex},
               byte_ratio={k: round(v / streamed, 4) for k, v in bytes_ex.items()},
               ratio_by_round={k: [round(a / b, 4) for a, b in zip(meas[k], meas["pair_eval_kind1"])] for k in bytes_ex})
print(f"lattice {'x'.join(map(str, shape))} dim={dim} n={n} Kr={kr} Ke={ke} (create {t_create:.1f} s): " +
      "; ".join(f"{k.replace('_', ' ')} {med[k]:.3f} ms ({gb[k] / med[k]:.2f} TB/s of {gb[k]:.2f} GB, {100 * gb[k] / med[k] / HBM_PEAK_TBS:.0f} % of the "
                f"HBM peak, x{med[k] / med['edge_eval_kind2']:.2f} the scalar time)" for k in med) + f"; spread over {rounds} rounds {100 * spread:.1f} %")
print(json.dumps(res))
if out_json:
    with open(out_json, "w") as fh:
        json.dump(res, fh, indent=1)
