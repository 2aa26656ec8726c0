// Sparse symmetric Hessian couplings (lfpsqp_sphess): the device object and its descriptor for the kernels of projcg.hip.
#pragma once
#include "internal.h"

// The symmetric off-diagonal part S of A = a0*I + diag(dg) + S, stored twice in ELL form (slot k of either form: one index and one value array
// of npad entries, so lanes walking consecutive rows of a slot are coalesced):
//   by ROWS  (Kr slots): the neighbours of row i in increasing index order -- the products; an empty slot holds i itself and 0.0;
//   by EDGES (Ke slots): every undirected edge once, at its owner -- the set-up of the reduced operator; an empty slot holds i and 0.0.
// Pad rows (n .. npad - 1) hold the index 0 and 0.0.
// Handles made by lfpsqp_sphess_like share the two index arrays (the PATTERN) and own their value arrays: the pattern is freed with the last of them.
struct lfpsqp_sphess {
    int64_t n = 0, nedges = 0;
    int Kr = 0, Ke = 0;
    int64_t npad = 0;               // round_up(n + 1, kPadRows): the length of the set-up vectors of the reduced operator (projcg.hip)
    int32_t* ridx = nullptr;        // [max(Kr, 1)][npad]
    double* rval = nullptr;
    int32_t* eidx = nullptr;        // [max(Ke, 1)][npad]
    double* eval = nullptr;
    mutable int* pattern_refs = nullptr;   // host counter of the handles on ridx / eidx; nullptr: this handle alone (never shared)
    // lfpsqp_sphess_create_points: rows dim*p + c, c < dim, are the components of point p < npoints (sphess_pair.hip); 0 / 0 for every other handle
    struct Points { int64_t npoints = 0; int dim = 0; } pts;
};

// Fixed points a_k that points of a handle of lfpsqp_sphess_create_points are tied to (lfpsqp_anchors_create), in ELL form BY SCALAR ROW as the
// handle itself: `width` slots (the most anchors on one point) of npad entries.  Row dim*p + c of slot k holds component c of the position of the
// k-th anchor of point p (in the order of the list) and copies of that anchor's weight and parameter; an empty slot (and every row behind the
// points) holds 0.0 in all three.  The object keeps the four numbers of the handle it was made for and no reference on it.
struct lfpsqp_anchors {
    int64_t n = 0, npoints = 0, npad = 0;
    int dim = 0;
    int64_t nanchors = 0;
    int width = 0;
    double* pos = nullptr;          // [max(width, 1)][npad]
    double* u = nullptr;
    double* par = nullptr;          // nullptr: created without parameters (every anchor uses the call's delta)
};

namespace lfpsqp {

// The row form as a kernel argument, with the interface of DiagsD (projcg.hip): the operator over vectors of n rows, couplings on the first nc.
struct SpHessD {
    double a0;
    const double* dg;
    const int32_t* idx;
    const double* val;
    int64_t npad;
    int64_t n;
    int64_t nc;
    int K;
    // row j < nc of the off-diagonal part applied to the vector whose entry r is src(r): the row's slots in slot order (increasing neighbour index)
    template <class SRC>
    __device__ __forceinline__ double couple(int64_t j, double o, SRC&& src) const {
        const int32_t* ip = idx + j;
        const double* vp = val + j;
#pragma unroll 4
        for (int k = 0; k < K; ++k) o = fma(vp[(int64_t)k * npad], src((int64_t)ip[(int64_t)k * npad]), o);
        return o;
    }
};

// ---- The producers of values for a handle (sphess_edge.hip, sphess_pair.hip, sphess_values.hip): vector kernels whose lanes own the rows (i, i + 1).
// p[o + i] is row i's entry of the slot at offset o = k * npad (o = 0: a vector).

// both rows live: one 16-byte store; else row i alone (the pad row behind an odd n is computed and dropped)
__device__ __forceinline__ void store_rows(double* p, int64_t i, int64_t o, bool v1, double a0, double a1) {
    if (v1) st2(p + i + o, make_double2(a0, a1));
    else p[i + o] = a0;
}
// either row may have nothing to store
__device__ __forceinline__ void store_rows(double* p, int64_t i, int64_t o, bool s0, bool s1, double a0, double a1) {
    if (s0 && s1) st2(p + i + o, make_double2(a0, a1));
    else if (s0) p[i + o] = a0;
    else if (s1) p[i + 1 + o] = a1;
}
// p[i] = fma(scale, a, p[i]) for both rows, or for row i alone: the read-modify-write of grad / diag
__device__ __forceinline__ void add_rows(double* p, int64_t i, bool v1, double scale, double a0, double a1) {
    if (v1) { const double2 r = ld2(p + i); st2(p + i, make_double2(fma(scale, a0, r.x), fma(scale, a1, r.y))); }
    else p[i] = fma(scale, a0, p[i]);
}

// The skeleton of an *_eval entry point: check, launch, finish.  The energy of the rows is reduced into one slot of the context's scalars.
inline double* eval_red(lfpsqp_ctx* ctx) { return ctx->scal + 32; }

// What the entry points share of their argument rules, for `nrows` live rows of W (the caller has checked ctx, W and x for NULL); *f = 0 until
// eval_finish sets it.
inline int eval_check(lfpsqp_ctx* ctx, const char* entry, const lfpsqp_sphess* W, int64_t nrows, const lfpsqp_vec* x, double* f, const lfpsqp_vec* grad,
                      const lfpsqp_vec* diag, const lfpsqp_sphess* H) {
    LF_ARG(ctx, x->n >= nrows);
    LF_ARG(ctx, (!grad || (grad->n >= nrows && grad->p != x->p)) && (!diag || (diag->n >= nrows && diag->p != x->p)) && (!grad || !diag || grad->p != diag->p));
    // H: another handle on W's pattern (W itself would lose the weights it is evaluated from)
    LF_ARG(ctx, !H || (H != W && H->ridx == W->ridx && H->eidx == W->eidx && H->rval != W->rval));
    if (ctx->comm_active())        // (a rank sees its own rows only: the edges across the shard boundaries would silently drop out)
        return set_err(ctx, LFPSQP_ERR_UNSUPPORTED, "%s: one rank only (no halo exchange between row shards)", entry);
    if (f) *f = 0.0;
    return 0;
}

// The launches: ROW<WF, WV, P...>{row..., grad, diag, hval} over W's row form -- WF: the rows' energy goes to eval_red; WV: grad / diag / H's row
// values are written, each optional; <WF, !WV> reads only -- then `own` over the edge form, when H is given and has one.
template <template <bool, bool, int...> class ROW, int... P, class OWN, class... A>
int eval_launch(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, bool wantf, double* grad, double* diag, lfpsqp_sphess* H, const OWN& own, A... row) {
    if (wantf && !(grad || diag || H))
        return run_vec<ROW<true, false, P...>, 1, NoPost>(ctx, W->n, ROW<true, false, P...>{row..., nullptr, nullptr, nullptr}, 0u, eval_red(ctx), NoPost());
    double* hr = H ? H->rval : nullptr;
    if (wantf) LF_TRY((run_vec<ROW<true, true, P...>, 1, NoPost>(ctx, W->n, ROW<true, true, P...>{row..., grad, diag, hr}, 0u, eval_red(ctx), NoPost())));
    else LF_TRY((run_vec<ROW<false, true, P...>, 0, NoPost>(ctx, W->n, ROW<false, true, P...>{row..., grad, diag, hr}, 0u, nullptr, NoPost())));
    if (H && W->Ke > 0) LF_TRY((run_vec<OWN, 0, NoPost>(ctx, W->n, own, 0u, nullptr, NoPost())));
    return 0;
}

// every edge is seen from both ends: the sum is halved here
inline int eval_finish(lfpsqp_ctx* ctx, double scale, double* f) {
    if (!f) return 0;
    double s = 0.0;
    LF_TRY(read_back(ctx, eval_red(ctx), &s, 1));
    *f = scale * (0.5 * s);
    return 0;
}

}  // namespace lfpsqp
