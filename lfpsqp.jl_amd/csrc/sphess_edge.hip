// lfpsqp_sphess_edge_eval: a NON-QUADRATIC edge term  scale * sum_e w_e psi(x_i - x_j)  over the pattern of an lfpsqp_sphess -- its value, its
// gradient, the diagonal sum_e w_e psi'' and the off-diagonal values -(scale w_e) psi'' written into BOTH ELL forms of a second handle on the same
// pattern (lfpsqp_sphess_like), which the solver kernels of projcg.hip then read as they read any handle: nothing there caches values.
//   kind 0: psi = t^2/2                  psi' = t                     psi'' = 1
//   kind 1: psi = t^2/2 + t^4/4          psi' = t + t^3               psi'' = 1 + 3 t^2
//   kind 2: psi = t^2 / (sqrt(1+u^2)+1)  psi' = t / sqrt(1+u^2)       psi'' = 1 / ((1+u^2) sqrt(1+u^2)),   u = t / delta   (pseudo-Huber)
// psi'' is a function of q = t*t alone: fl(x_i - x_j) = -fl(x_j - x_i), so both endpoints of an edge, and the row and the edge form, compute the
// same q and store the same bits -- the symmetry the set-up of the reduced operator relies on.  Roundings per value, t = fl(x_i - x_j) against the
// exact difference (tests/test_sphess_edge.py holds the kernels to these counts): q 3; kind 1: psi 7, psi' 5, psi'' 4; kind 2 (1/delta^2 formed on the
// host: 2): 1+u^2 6, its root 4, psi 9, psi' 6, psi'' 12; a stored value two more (scale*w and the product).
#include <math.h>

#include "sphess.h"

namespace lfpsqp {

template <int KIND>
struct EdgePot {
    double rd2;                // 1 / delta^2 (kind 2)
    // (psi, psi', psi'') at t, q = t*t; only what the caller uses is kept by the compiler
    __device__ __forceinline__ void eval(double t, double q, double& p0, double& p1, double& p2) const {
        if (KIND == 0) {
            p0 = 0.5 * q; p1 = t; p2 = 1.0;
        } else if (KIND == 1) {
            p0 = fma(0.25 * q, q, 0.5 * q); p1 = fma(q, t, t); p2 = fma(3.0, q, 1.0);
        } else {
            const double a = fma(q, rd2, 1.0), s = sqrt(a);
            p0 = q / (s + 1.0); p1 = t / s; p2 = 1.0 / (a * s);
        }
    }
};

// Row form, two rows per lane: per slot one gather of x, one fma into each of the row's sums, the new value stored into H's row slot.  WF: the row's
// energy goes to the reduction (every edge is seen from both ends: the host halves the sum); WV: grad / diag / hval, each optional.  <WF, !WV> reads
// indices, weights and x and writes nothing.  Empty slots (the row itself, weight 0) have t = 0 and add 0; the pad row behind an odd n is computed
// and dropped.  The slot loop is unrolled by four for kind 0, as SpHessD::couple, and rolled for the other kinds: unrolled, the two rows' division and
// square-root sequences take 100 .. 124 VGPRs (4 waves per SIMD); rolled 46 .. 68 (7 or 8, like DiagsMulF<SpHessD>), no scratch either way.
template <bool WF, bool WV, int KIND>
struct EdgeRowF {
    EdgePot<KIND> pot;
    const int32_t* idx;
    const double* w;
    int64_t npad;
    int K;
    const double* x;
    double scale;
    double* grad;
    double* diag;
    double* hval;
    __device__ __forceinline__ bool skip() const { return false; }
    __device__ __forceinline__ void apply(int64_t i, bool v0, bool v1, double* red) const {
        if (!v0) return;
        const double2 xi = ld2(x + i);
        const int32_t* ip = idx + i;
        const double* wp = w + i;
        double e0 = 0.0, e1 = 0.0, g0 = 0.0, g1 = 0.0, d0 = 0.0, d1 = 0.0;
#pragma unroll(KIND == 0 ? 4 : 1)
        for (int k = 0; k < K; ++k) {
            const int64_t o = (int64_t)k * npad;
            const int2 jj = *reinterpret_cast<const int2*>(ip + o);
            const double2 ww = ld2(wp + o);
            const double t0 = xi.x - x[jj.x], t1 = xi.y - x[jj.y];
            double a0, b0, c0, a1, b1, c1;
            pot.eval(t0, t0 * t0, a0, b0, c0);
            pot.eval(t1, t1 * t1, a1, b1, c1);
            if (WF) { e0 = fma(ww.x, a0, e0); e1 = fma(ww.y, a1, e1); }
            if (WV) {
                g0 = fma(ww.x, b0, g0); g1 = fma(ww.y, b1, g1);
                d0 = fma(ww.x, c0, d0); d1 = fma(ww.y, c1, d1);
                if (hval) {
                    const double h0 = -((scale * ww.x) * c0), h1 = -((scale * ww.y) * c1);
                    store_rows(hval, i, o, v1, h0, h1);
                }
            }
        }
        if (WF) red[0] += e0 + (v1 ? e1 : 0.0);
        if (WV) {
            if (grad) add_rows(grad, i, v1, scale, g0, g1);
            if (diag) add_rows(diag, i, v1, scale, d0, d1);
        }
    }
};

// Edge form: slot k of owner o holds the partner p and w; the same expression from x_o - x_p
template <int KIND>
struct EdgeOwnF {
    EdgePot<KIND> pot;
    const int32_t* idx;
    const double* w;
    int64_t npad;
    int K;
    const double* x;
    double scale;
    double* hval;
    __device__ __forceinline__ bool skip() const { return false; }
    __device__ __forceinline__ void apply(int64_t i, bool v0, bool v1, double*) const {
        if (!v0) return;
        const double2 xi = ld2(x + i);
        const int32_t* ip = idx + i;
        const double* wp = w + i;
#pragma unroll(KIND == 0 ? 4 : 1)
        for (int k = 0; k < K; ++k) {
            const int64_t o = (int64_t)k * npad;
            const int2 jj = *reinterpret_cast<const int2*>(ip + o);
            const double2 ww = ld2(wp + o);
            const double t0 = xi.x - x[jj.x], t1 = xi.y - x[jj.y];
            double a0, b0, c0, a1, b1, c1;
            pot.eval(t0, t0 * t0, a0, b0, c0);
            pot.eval(t1, t1 * t1, a1, b1, c1);
            const double h0 = -((scale * ww.x) * c0), h1 = -((scale * ww.y) * c1);
            // (store_rows, written out: through the helper the compiler issues this loop's loads of kinds 0 and 1 in another order)
            if (v1) st2(hval + i + o, make_double2(h0, h1));
            else hval[i + o] = h0;
        }
    }
};

template <int KIND>
static int edge_eval_kind(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, double rd2, double scale, const double* x, bool wantf, double* grad, double* diag,
                          lfpsqp_sphess* H) {
    const EdgePot<KIND> pot{rd2};
    return eval_launch<EdgeRowF, KIND>(ctx, W, wantf, grad, diag, H, EdgeOwnF<KIND>{pot, W->eidx, W->eval, W->npad, W->Ke, x, scale, H ? H->eval : nullptr},
                                       pot, W->ridx, W->rval, W->npad, W->Kr, x, scale);
}

}  // namespace lfpsqp

using namespace lfpsqp;

extern "C" int lfpsqp_sphess_edge_eval(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, int kind, double delta, double scale, const lfpsqp_vec* x, double* f,
                                       lfpsqp_vec* grad, lfpsqp_vec* diag, lfpsqp_sphess* H) {
    LF_ARG(ctx, ctx && W && x && kind >= 0 && kind <= 2 && std::isfinite(scale));
    LF_ARG(ctx, kind != 2 || (std::isfinite(delta) && delta > 0.0));
    LF_TRY(eval_check(ctx, "lfpsqp_sphess_edge_eval", W, W->n, x, f, grad, diag, H));
    if (W->n == 0 || !(f || grad || diag || H)) return 0;
    const double rd2 = kind == 2 ? 1.0 / (delta * delta) : 0.0;
    double *gp = grad ? grad->p : nullptr, *dp = diag ? diag->p : nullptr;
    if (kind == 0) LF_TRY(edge_eval_kind<0>(ctx, W, rd2, scale, x->p, f != nullptr, gp, dp, H));
    else if (kind == 1) LF_TRY(edge_eval_kind<1>(ctx, W, rd2, scale, x->p, f != nullptr, gp, dp, H));
    else LF_TRY(edge_eval_kind<2>(ctx, W, rd2, scale, x->p, f != nullptr, gp, dp, H));
    return eval_finish(ctx, scale, f);
}
