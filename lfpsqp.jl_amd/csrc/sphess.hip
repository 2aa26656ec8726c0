// lfpsqp_sphess: a symmetric sparse Hessian's off-diagonal part, built once on the host from triplets into the two ELL forms of sphess.h.
// The kernels that read them live with the solver (projcg.hip: products, gathers, set-up weights) and with the Gram kernel (factorize.hip: the
// gathered operand).
#include <math.h>

#include <algorithm>
#include <vector>

#include "sphess.h"

using namespace lfpsqp;

namespace {
struct Edge {
    int32_t i, j;       // i < j
    double v;
};
}  // namespace

extern "C" {

int lfpsqp_sphess_create(lfpsqp_ctx* ctx, int64_t n, int64_t nnz, const int64_t* rows, const int64_t* cols, const double* vals, lfpsqp_sphess** out) {
    LF_ARG(ctx, ctx && out && n >= 0 && nnz >= 0 && (nnz == 0 || (rows && cols && vals)));
    *out = nullptr;
    if (n >= ((int64_t)1 << 31)) return set_err(ctx, LFPSQP_ERR_UNSUPPORTED, "sphess: %lld rows (indices are stored as int32)", (long long)n);
    std::vector<Edge> ed((size_t)nnz);
    bool sorted = true;
    for (int64_t e = 0; e < nnz; ++e) {
        const int64_t i = rows[e], j = cols[e];
        if (i < 0 || i >= n || j < 0 || j >= n) return set_err(ctx, LFPSQP_ERR_ARG, "sphess: entry %lld out of range", (long long)e);
        if (i == j) return set_err(ctx, LFPSQP_ERR_ARG, "sphess: entry %lld lies on the diagonal (the diagonal is dg)", (long long)e);
        if (!std::isfinite(vals[e])) return set_err(ctx, LFPSQP_ERR_ARG, "sphess: entry %lld is not finite", (long long)e);
        ed[(size_t)e] = Edge{(int32_t)std::min(i, j), (int32_t)std::max(i, j), vals[e]};
        if (e > 0 && sorted) {
            const Edge& p = ed[(size_t)e - 1];
            sorted = p.i < ed[(size_t)e].i || (p.i == ed[(size_t)e].i && p.j <= ed[(size_t)e].j);
        }
    }
    // lexicographic (i, j), i < j; duplicates (a mirrored (j, i) included) add up in the order they were given; a sum of zero keeps its slot
    if (!sorted) std::stable_sort(ed.begin(), ed.end(), [](const Edge& a, const Edge& b) { return a.i != b.i ? a.i < b.i : a.j < b.j; });
    size_t ne = 0;
    for (size_t e = 0; e < ed.size(); ++e) {
        if (ne > 0 && ed[ne - 1].i == ed[e].i && ed[ne - 1].j == ed[e].j) ed[ne - 1].v += ed[e].v;
        else ed[ne++] = ed[e];
    }
    ed.resize(ne);
    std::vector<int32_t> deg((size_t)std::max<int64_t>(n, 1), 0), own((size_t)std::max<int64_t>(n, 1), 0);
    std::vector<uint8_t> at_j(ne, 0);
    int Kr = 0, Ke = 0;
    for (size_t e = 0; e < ne; ++e) {
        const int32_t i = ed[e].i, j = ed[e].j;
        Kr = std::max(Kr, std::max(++deg[(size_t)i], ++deg[(size_t)j]));
        // the owner: j if it owns strictly fewer edges so far, otherwise i
        at_j[e] = own[(size_t)j] < own[(size_t)i];
        Ke = std::max(Ke, ++own[(size_t)(at_j[e] ? j : i)]);
    }
    if (Kr > LFPSQP_SPHESS_MAX_ROW)
        return set_err(ctx, LFPSQP_ERR_UNSUPPORTED, "sphess: a row with %d off-diagonal entries (> %d)", Kr, LFPSQP_SPHESS_MAX_ROW);
    lfpsqp_sphess* S = new lfpsqp_sphess();
    S->n = n; S->nedges = (int64_t)ne; S->Kr = Kr; S->Ke = Ke;
    S->npad = round_up((n > 0 ? n : 1) + 1, kPadRows);
    const size_t npad = (size_t)S->npad, rsz = (size_t)std::max(Kr, 1) * npad, esz = (size_t)std::max(Ke, 1) * npad;
    std::vector<int32_t> ri(rsz, 0), ei(esz, 0);
    std::vector<double> rv(rsz, 0.0), ev(esz, 0.0);
    for (int64_t r = 0; r < n; ++r) {
        for (int k = 0; k < std::max(Kr, 1); ++k) ri[(size_t)k * npad + (size_t)r] = (int32_t)r;
        for (int k = 0; k < std::max(Ke, 1); ++k) ei[(size_t)k * npad + (size_t)r] = (int32_t)r;
    }
    // (in lexicographic order every edge (i, r), i < r, comes before every edge (r, j), r < j: a row's slots fill in increasing neighbour order)
    std::fill(deg.begin(), deg.end(), 0);
    std::fill(own.begin(), own.end(), 0);
    for (size_t e = 0; e < ne; ++e) {
        const int32_t i = ed[e].i, j = ed[e].j;
        const size_t si = (size_t)deg[(size_t)i]++ * npad + (size_t)i, sj = (size_t)deg[(size_t)j]++ * npad + (size_t)j;
        ri[si] = j; rv[si] = ed[e].v;
        ri[sj] = i; rv[sj] = ed[e].v;
        const int32_t o = at_j[e] ? j : i, p = at_j[e] ? i : j;
        const size_t so = (size_t)own[(size_t)o]++ * npad + (size_t)o;
        ei[so] = p; ev[so] = ed[e].v;
    }
    bool ok = true;
    auto dev_copy = [&](void** dst, const void* src, size_t bytes) {
        if (!ok) return;
        ok = hipMalloc(dst, bytes) == hipSuccess;
        if (ok) ok = hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    };
    dev_copy((void**)&S->ridx, ri.data(), rsz * sizeof(int32_t));
    dev_copy((void**)&S->rval, rv.data(), rsz * sizeof(double));
    dev_copy((void**)&S->eidx, ei.data(), esz * sizeof(int32_t));
    dev_copy((void**)&S->eval, ev.data(), esz * sizeof(double));
    if (ok) ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) {
        lfpsqp_sphess_free(ctx, S);
        return set_err(ctx, LFPSQP_ERR_HIP, "sphess: device allocation / upload failed");
    }
    *out = S;
    return 0;
}

// Points with dim unknowns each, interleaved (row dim*p + c): a point edge becomes its dim^2 scalar entries, every point gets the dim (dim - 1) / 2
// entries between its own components (value 0.0: the slot stays), and the builder above does the rest.
int lfpsqp_sphess_create_points(lfpsqp_ctx* ctx, int64_t n, int64_t npoints, int dim, int64_t nedges, const int64_t* pi, const int64_t* pj,
                                const double* w, lfpsqp_sphess** out) {
    LF_ARG(ctx, ctx && out && npoints >= 0 && nedges >= 0 && (nedges == 0 || (pi && pj && w)));
    *out = nullptr;
    LF_ARG(ctx, dim == 2 || dim == 3);
    if (npoints >= ((int64_t)1 << 31) / dim) return set_err(ctx, LFPSQP_ERR_UNSUPPORTED, "sphess: %lld points of %d unknowns (indices are stored as int32)", (long long)npoints, dim);
    LF_ARG(ctx, n >= dim * npoints);
    std::vector<std::pair<int64_t, int64_t>> pe((size_t)nedges);
    for (int64_t e = 0; e < nedges; ++e) {
        const int64_t p = pi[e], q = pj[e];
        if (p < 0 || p >= npoints || q < 0 || q >= npoints) return set_err(ctx, LFPSQP_ERR_ARG, "sphess: point edge %lld out of range", (long long)e);
        if (p == q) return set_err(ctx, LFPSQP_ERR_ARG, "sphess: point edge %lld joins a point to itself", (long long)e);
        if (!std::isfinite(w[e])) return set_err(ctx, LFPSQP_ERR_ARG, "sphess: point edge %lld is not finite", (long long)e);
        pe[(size_t)e] = {std::min(p, q), std::max(p, q)};
    }
    // the distinct neighbours of a point: its scalar rows hold dim of them each, and the dim - 1 entries of the point itself
    std::sort(pe.begin(), pe.end());
    pe.erase(std::unique(pe.begin(), pe.end()), pe.end());
    std::vector<int32_t> deg((size_t)std::max<int64_t>(npoints, 1), 0);
    int degmax = 0;
    for (const auto& e : pe) degmax = std::max(degmax, std::max(++deg[(size_t)e.first], ++deg[(size_t)e.second]));
    const int limit = (LFPSQP_SPHESS_MAX_ROW - (dim - 1)) / dim;
    if (degmax > limit)
        return set_err(ctx, LFPSQP_ERR_UNSUPPORTED, "sphess: a point with %d neighbours (> %d with %d unknowns per point: %d entries per row)", degmax, limit,
                       dim, LFPSQP_SPHESS_MAX_ROW);
    const size_t nnz = (size_t)nedges * (size_t)(dim * dim) + (size_t)npoints * (size_t)(dim * (dim - 1) / 2);
    std::vector<int64_t> rows(nnz), cols(nnz);
    std::vector<double> vals(nnz);
    size_t z = 0;
    for (int64_t p = 0; p < npoints; ++p)
        for (int c = 0; c < dim; ++c)
            for (int d = c + 1; d < dim; ++d, ++z) { rows[z] = dim * p + c; cols[z] = dim * p + d; vals[z] = 0.0; }
    for (int64_t e = 0; e < nedges; ++e)             // (in the order given: every entry of a pair sums its duplicates in the same order, to the same bits)
        for (int c = 0; c < dim; ++c)
            for (int d = 0; d < dim; ++d, ++z) { rows[z] = dim * pi[e] + c; cols[z] = dim * pj[e] + d; vals[z] = w[e]; }
    LF_TRY(lfpsqp_sphess_create(ctx, n, (int64_t)nnz, rows.data(), cols.data(), vals.data(), out));
    (*out)->pts.npoints = npoints;
    (*out)->pts.dim = dim;
    return 0;
}

int lfpsqp_sphess_points_info(const lfpsqp_sphess* S, int64_t* npoints, int64_t* dim) {
    if (!S) return LFPSQP_ERR_ARG;
    if (npoints) *npoints = S->pts.npoints;
    if (dim) *dim = S->pts.dim;
    return 0;
}

int lfpsqp_sphess_free(lfpsqp_ctx* ctx, lfpsqp_sphess* S) {
    if (!S) return 0;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    bool last = true;                                   // the pattern goes with the last handle on it
    if (S->pattern_refs) {
        last = --*S->pattern_refs == 0;
        if (last) delete S->pattern_refs;
    }
    for (void* p : {last ? (void*)S->ridx : nullptr, (void*)S->rval, last ? (void*)S->eidx : nullptr, (void*)S->eval})
        if (p) (void)hipFree(p);
    delete S;
    return 0;
}

int lfpsqp_sphess_like(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, lfpsqp_sphess** out) {
    LF_ARG(ctx, ctx && W && out);
    *out = nullptr;
    lfpsqp_sphess* H = new lfpsqp_sphess(*W);
    H->rval = H->eval = nullptr;
    H->pattern_refs = nullptr;                          // (until the copies stand: freeing H then leaves W's pattern alone)
    H->ridx = H->eidx = nullptr;
    const size_t npad = (size_t)W->npad, rsz = (size_t)std::max(W->Kr, 1) * npad, esz = (size_t)std::max(W->Ke, 1) * npad;
    bool ok = hipMalloc((void**)&H->rval, rsz * sizeof(double)) == hipSuccess && hipMalloc((void**)&H->eval, esz * sizeof(double)) == hipSuccess;
    if (ok) ok = hipMemcpyAsync(H->rval, W->rval, rsz * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess;
    if (ok) ok = hipMemcpyAsync(H->eval, W->eval, esz * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess;
    if (ok) ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) {
        lfpsqp_sphess_free(ctx, H);
        return set_err(ctx, LFPSQP_ERR_HIP, "sphess: device allocation / copy failed");
    }
    if (!W->pattern_refs) W->pattern_refs = new int(1);
    ++*W->pattern_refs;
    H->pattern_refs = W->pattern_refs;
    H->ridx = W->ridx;
    H->eidx = W->eidx;
    *out = H;
    return 0;
}

// One value per point edge of W as a handle on W's pattern: a PARAMETER (a rest length), so nothing adds up -- the list must name every point edge
// of W exactly once.  The list is checked against W's row form read back from the device; the value arrays are then those of a temporary handle
// built from the same list (the builder is deterministic in the edge set, so its layout is W's: compared, index by index), copied into a _like
// handle of W.
int lfpsqp_sphess_points_values(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, int64_t nedges, const int64_t* pi, const int64_t* pj, const double* vals,
                                lfpsqp_sphess** out) {
    LF_ARG(ctx, ctx && W && out && nedges >= 0 && (nedges == 0 || (pi && pj && vals)));
    *out = nullptr;
    LF_ARG(ctx, W->pts.dim == 2 || W->pts.dim == 3);             // a handle of lfpsqp_sphess_create_points (or a handle on its pattern)
    const int dim = W->pts.dim;
    const int64_t npoints = W->pts.npoints;
    const size_t npad = (size_t)W->npad, rsz = (size_t)std::max(W->Kr, 1) * npad, esz = (size_t)std::max(W->Ke, 1) * npad;
    std::vector<int32_t> ri(rsz), ei(esz);
    LF_HIP(ctx, hipMemcpyAsync(ri.data(), W->ridx, rsz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    LF_HIP(ctx, hipMemcpyAsync(ei.data(), W->eidx, esz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // q is a neighbour of p: component 0 of q sits in row dim*p
    auto joined = [&](int64_t p, int64_t q) {
        for (int k = 0; k < W->Kr; ++k)
            if (ri[(size_t)k * npad + (size_t)(dim * p)] == (int32_t)(dim * q)) return true;
        return false;
    };
    struct Named { int64_t p, q, e; };
    std::vector<Named> pe((size_t)nedges);
    for (int64_t e = 0; e < nedges; ++e) {
        const int64_t p = pi[e], q = pj[e];
        if (p < 0 || p >= npoints || q < 0 || q >= npoints) return set_err(ctx, LFPSQP_ERR_ARG, "sphess: point edge %lld out of range", (long long)e);
        if (!std::isfinite(vals[e]) || vals[e] < 0.0) return set_err(ctx, LFPSQP_ERR_ARG, "sphess: the value of point edge %lld is not finite or negative", (long long)e);
        if (p == q || !joined(p, q)) return set_err(ctx, LFPSQP_ERR_ARG, "sphess: point edge %lld is no edge of the handle", (long long)e);
        pe[(size_t)e] = Named{std::min(p, q), std::max(p, q), e};
    }
    std::sort(pe.begin(), pe.end(), [](const Named& a, const Named& b) { return a.p != b.p ? a.p < b.p : a.q != b.q ? a.q < b.q : a.e < b.e; });
    for (size_t k = 1; k < pe.size(); ++k)
        if (pe[k].p == pe[k - 1].p && pe[k].q == pe[k - 1].q)
            return set_err(ctx, LFPSQP_ERR_ARG, "sphess: point edge %lld repeats point edge %lld (a parameter does not add up)", (long long)pe[k].e,
                           (long long)pe[k - 1].e);
    const int64_t have = (W->nedges - npoints * (dim * (dim - 1) / 2)) / (dim * dim);
    if (nedges != have)
        return set_err(ctx, LFPSQP_ERR_ARG, "sphess: %lld of the handle's %lld point edges are missing a value", (long long)(have - nedges), (long long)have);
    lfpsqp_sphess* T = nullptr;
    LF_TRY(lfpsqp_sphess_create_points(ctx, W->n, npoints, dim, nedges, pi, pj, vals, &T));
    bool same = T->Kr == W->Kr && T->Ke == W->Ke && T->npad == W->npad && T->nedges == W->nedges;
    if (same) {
        std::vector<int32_t> tr(rsz), te(esz);
        same = hipMemcpyAsync(tr.data(), T->ridx, rsz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
               hipMemcpyAsync(te.data(), T->eidx, esz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
               hipStreamSynchronize(ctx->stream) == hipSuccess && tr == ri && te == ei;
    }
    lfpsqp_sphess* P = nullptr;
    int rc = same ? lfpsqp_sphess_like(ctx, W, &P) : set_err(ctx, LFPSQP_ERR_ARG, "sphess: the point edges do not give the handle's layout");
    if (rc == 0) {
        const bool ok = hipMemcpyAsync(P->rval, T->rval, rsz * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess &&
                        hipMemcpyAsync(P->eval, T->eval, esz * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess &&
                        hipStreamSynchronize(ctx->stream) == hipSuccess;
        if (!ok) {
            lfpsqp_sphess_free(ctx, P);
            rc = set_err(ctx, LFPSQP_ERR_HIP, "sphess: device copy failed");
        }
    }
    lfpsqp_sphess_free(ctx, T);
    if (rc == 0) *out = P;
    return rc;
}

int lfpsqp_anchors_create(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, int64_t nanchors, const int64_t* point, const double* pos, const double* u,
                          const double* par, lfpsqp_anchors** out) {
    LF_ARG(ctx, ctx && W && out && nanchors >= 0 && (nanchors == 0 || (point && pos && u)));
    *out = nullptr;
    LF_ARG(ctx, W->pts.dim == 2 || W->pts.dim == 3);             // a handle of lfpsqp_sphess_create_points (or a handle on its pattern)
    const int dim = W->pts.dim;
    const int64_t npoints = W->pts.npoints;
    std::vector<int32_t> cnt((size_t)std::max<int64_t>(npoints, 1), 0);
    int width = 0;
    for (int64_t k = 0; k < nanchors; ++k) {
        if (point[k] < 0 || point[k] >= npoints) return set_err(ctx, LFPSQP_ERR_ARG, "anchors: the point of anchor %lld is out of range", (long long)k);
        bool fin = std::isfinite(u[k]) && (!par || std::isfinite(par[k]));
        for (int c = 0; c < dim; ++c) fin = fin && std::isfinite(pos[dim * k + c]);
        if (!fin) return set_err(ctx, LFPSQP_ERR_ARG, "anchors: anchor %lld has a position, a weight or a parameter that is not finite", (long long)k);
        if (par && par[k] < 0.0) return set_err(ctx, LFPSQP_ERR_ARG, "anchors: the parameter of anchor %lld is negative", (long long)k);
        width = std::max(width, ++cnt[(size_t)point[k]]);
    }
    if (width > LFPSQP_ANCHORS_MAX_POINT)
        return set_err(ctx, LFPSQP_ERR_UNSUPPORTED, "anchors: a point with %d anchors (> %d)", width, LFPSQP_ANCHORS_MAX_POINT);
    const size_t npad = (size_t)W->npad, sz = (size_t)std::max(width, 1) * npad;
    std::vector<double> hp(sz, 0.0), hu(sz, 0.0), hr(par ? sz : 0, 0.0);
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int64_t k = 0; k < nanchors; ++k) {
        const size_t s = (size_t)cnt[(size_t)point[k]]++ * npad + (size_t)(dim * point[k]);
        for (int c = 0; c < dim; ++c) {
            hp[s + (size_t)c] = pos[dim * k + c];
            hu[s + (size_t)c] = u[k];
            if (par) hr[s + (size_t)c] = par[k];
        }
    }
    lfpsqp_anchors* A = new lfpsqp_anchors();
    A->n = W->n; A->npoints = npoints; A->npad = W->npad; A->dim = dim; A->nanchors = nanchors; A->width = width;
    bool ok = true;
    auto dev_copy = [&](double** dst, const std::vector<double>& src) {
        if (!ok) return;
        ok = hipMalloc((void**)dst, src.size() * sizeof(double)) == hipSuccess;
        if (ok) ok = hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    };
    dev_copy(&A->pos, hp);
    dev_copy(&A->u, hu);
    if (par) dev_copy(&A->par, hr);
    if (ok) ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) {
        lfpsqp_anchors_free(ctx, A);
        return set_err(ctx, LFPSQP_ERR_HIP, "anchors: device allocation / upload failed");
    }
    *out = A;
    return 0;
}

int lfpsqp_anchors_free(lfpsqp_ctx* ctx, lfpsqp_anchors* A) {
    if (!A) return 0;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    for (void* p : {(void*)A->pos, (void*)A->u, (void*)A->par})
        if (p) (void)hipFree(p);
    delete A;
    return 0;
}

int lfpsqp_anchors_info(const lfpsqp_anchors* A, int64_t* nanchors, int64_t* width) {
    if (!A) return LFPSQP_ERR_ARG;
    if (nanchors) *nanchors = A->nanchors;
    if (width) *width = A->width;
    return 0;
}

int lfpsqp_sphess_info(const lfpsqp_sphess* S, int64_t* n, int64_t* nedges, int64_t* row_width, int64_t* edge_width) {
    if (!S) return LFPSQP_ERR_ARG;
    if (n) *n = S->n;
    if (nedges) *nedges = S->nedges;
    if (row_width) *row_width = S->Kr;
    if (edge_width) *edge_width = S->Ke;
    return 0;
}

}  // extern "C"
