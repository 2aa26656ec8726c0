// lfpsqp_sphess_map / lfpsqp_sphess_set_values: the STRUCTURE / VALUES interface of a sparse Lagrangian Hessian.  The caller declares a triplet
// pattern (rows, cols) once -- the map, built on the host against the pattern of an lfpsqp_sphess and uploaded -- and hands over nnz values before
// every solve; two vector kernels place them into BOTH ELL forms of a handle on that pattern and into the Hessian diagonal.  Per stored slot the
// map holds the position of the slot's FIRST triplet (-1: none) and, only where some position is named more than once, a `next` chain through
// the duplicates in the order given: the stored value is ((v_p0 + v_p1) + v_p2) ..., the sum lfpsqp_sphess_create forms for the same triplets, so
// a refreshed handle holds the bits of a freshly created one and the two forms of an edge hold the same bits.  Nothing here is read by the solver
// kernels of projcg.hip: like lfpsqp_sphess_edge_eval this is a producer of values for a handle on a shared pattern.
#include <algorithm>
#include <vector>

#include "sphess.h"

struct lfpsqp_sphess_map {
    int64_t n = 0, nnz = 0, ndiag = 0, max_dup = 0;
    int Kr = 0, Ke = 0;
    int64_t npad = 0;
    const int32_t* ridx = nullptr;      // the pattern this map was built on (shared with its handles; freed with the last holder)
    const int32_t* eidx = nullptr;
    int* pattern_refs = nullptr;
    int32_t* rsrc = nullptr;            // [max(Kr, 1)][npad]
    int32_t* esrc = nullptr;            // [max(Ke, 1)][npad]
    int32_t* dsrc = nullptr;            // [npad]
    int32_t* next = nullptr;            // [nnz], only with max_dup > 1
};

namespace lfpsqp {

// the chain sum of position p (-1: +0.0), starting from the first value
template <bool DUP>
__device__ __forceinline__ double chain_sum(const double* vals, const int32_t* next, int32_t p) {
    if (p < 0) return 0.0;
    double s = vals[p];
    if (DUP)
        for (int32_t q = next[p]; q >= 0; q = next[q]) s += vals[q];
    return s;
}

// Either form, two rows per lane: per slot one int2 of source positions, the gather of vals, one 16-byte store into H's slot; then the diagonal, which
// OVERWRITES.  hval == nullptr: the diagonal alone (K = 0); diag == nullptr: the slots alone.  The pad row behind an odd n holds -1 in every array
// of the map: its value is computed (+0.0) and dropped, a single store goes to row n - 1.  DUP = false reads no `next` and has no inner loop.
template <bool DUP>
struct ValRowF {
    const int32_t* src;
    const int32_t* dsrc;
    const int32_t* next;
    const double* vals;
    int64_t npad;
    int K;
    double* hval;
    double* diag;
    __device__ __forceinline__ bool skip() const { return false; }
    __device__ __forceinline__ void apply(int64_t i, bool v0, bool v1, double*) const {
        if (!v0) return;
        const int32_t* sp = src + i;
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
            const int64_t o = (int64_t)k * npad;
            const int2 pp = *reinterpret_cast<const int2*>(sp + o);
            const double h0 = chain_sum<DUP>(vals, next, pp.x), h1 = chain_sum<DUP>(vals, next, pp.y);
            store_rows(hval, i, o, v1, h0, h1);
        }
        if (diag) {
            const int2 pp = *reinterpret_cast<const int2*>(dsrc + i);
            const double d0 = chain_sum<DUP>(vals, next, pp.x), d1 = chain_sum<DUP>(vals, next, pp.y);
            store_rows(diag, i, 0, v1, d0, d1);
        }
    }
};

template <bool DUP>
static int set_values_launch(lfpsqp_ctx* ctx, const lfpsqp_sphess_map* M, const double* vals, double* diag, lfpsqp_sphess* H) {
    const bool rows = H && M->Kr > 0;
    if (rows || diag)
        LF_TRY((run_vec<ValRowF<DUP>, 0, NoPost>(
            ctx, M->n, ValRowF<DUP>{M->rsrc, M->dsrc, M->next, vals, M->npad, rows ? M->Kr : 0, rows ? H->rval : nullptr, diag}, 0u, nullptr, NoPost())));
    if (H && M->Ke > 0)                                 // the edge form: the same per owner slot, no diagonal
        LF_TRY((run_vec<ValRowF<DUP>, 0, NoPost>(ctx, M->n, ValRowF<DUP>{M->esrc, M->dsrc, M->next, vals, M->npad, M->Ke, H->eval, nullptr}, 0u, nullptr,
                                                  NoPost())));
    return 0;
}

}  // namespace lfpsqp

using namespace lfpsqp;

extern "C" {

int lfpsqp_sphess_map_free(lfpsqp_ctx* ctx, lfpsqp_sphess_map* M) {
    if (!M) return 0;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    bool last = false;                                  // the pattern goes with the last holder, a handle or a map
    if (M->pattern_refs) {
        last = --*M->pattern_refs == 0;
        if (last) delete M->pattern_refs;
    }
    for (void* p : {last ? (void*)M->ridx : nullptr, last ? (void*)M->eidx : nullptr, (void*)M->rsrc, (void*)M->esrc, (void*)M->dsrc, (void*)M->next})
        if (p) (void)hipFree(p);
    delete M;
    return 0;
}

int lfpsqp_sphess_map_create(lfpsqp_ctx* ctx, const lfpsqp_sphess* S, int64_t nnz, const int64_t* rows, const int64_t* cols, lfpsqp_sphess_map** out) {
    LF_ARG(ctx, ctx && S && out && nnz >= 0 && (nnz == 0 || (rows && cols)));
    *out = nullptr;
    if (nnz >= ((int64_t)1 << 31)) return set_err(ctx, LFPSQP_ERR_UNSUPPORTED, "sphess_map: %lld triplets (positions are stored as int32)", (long long)nnz);
    const int64_t n = S->n;
    const int Kr = S->Kr, Ke = S->Ke;
    const size_t npad = (size_t)S->npad, rsz = (size_t)std::max(Kr, 1) * npad, esz = (size_t)std::max(Ke, 1) * npad;
    // S's pattern, read back from the device (the handle keeps no host copy)
    std::vector<int32_t> ri(rsz), ei(esz);
    LF_HIP(ctx, hipMemcpyAsync(ri.data(), S->ridx, rsz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    LF_HIP(ctx, hipMemcpyAsync(ei.data(), S->eidx, esz * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> rs(rsz, -1), es(esz, -1), ds(npad, -1), nx((size_t)nnz, -1);
    // per chain (keyed by the row-form slot at the edge's lower endpoint, or by the row for the diagonal): its last position and its length
    std::vector<int32_t> rtail(rsz, -1), dtail(npad, -1), rlen(rsz, 0), dlen(npad, 0);
    int64_t ndiag = 0, max_dup = 0;
    for (int64_t p = 0; p < nnz; ++p) {
        const int64_t i = rows[p], j = cols[p];
        if (i < 0 || i >= n || j < 0 || j >= n) return set_err(ctx, LFPSQP_ERR_ARG, "sphess_map: entry %lld out of range", (long long)p);
        int32_t *head, *tail, *len;
        if (i == j) {
            ++ndiag;
            head = &ds[(size_t)i]; tail = &dtail[(size_t)i]; len = &dlen[(size_t)i];
        } else {
            const int64_t lo = std::min(i, j), hi = std::max(i, j);
            int k = 0;
            while (k < Kr && ri[(size_t)k * npad + (size_t)lo] != (int32_t)hi) ++k;
            if (k == Kr)
                return set_err(ctx, LFPSQP_ERR_ARG, "sphess_map: entry %lld (%lld, %lld) is not an edge of the pattern", (long long)p, (long long)i,
                               (long long)j);
            const size_t a = (size_t)k * npad + (size_t)lo;
            head = &rs[a]; tail = &rtail[a]; len = &rlen[a];
        }
        if (*head < 0) *head = (int32_t)p;
        else nx[(size_t)*tail] = (int32_t)p;
        *tail = (int32_t)p;
        max_dup = std::max<int64_t>(max_dup, ++*len);
    }
    // the other endpoint's row slot and the owner's edge slot of every edge, by the walk of lfpsqp_sphess_create: edges (i, j), i < j, in
    // lexicographic order fill a row's slots in increasing neighbour order, and the owner is j if it owns strictly fewer edges so far; each place
    // is checked against the indices read back
    {
        std::vector<int32_t> deg((size_t)std::max<int64_t>(n, 1), 0), own((size_t)std::max<int64_t>(n, 1), 0);
        for (int64_t i = 0; i < n; ++i) {
            for (int k = deg[(size_t)i]; k < Kr; ++k) {
                const size_t a = (size_t)k * npad + (size_t)i;
                const int32_t j = ri[a];
                if (j <= (int32_t)i) break;                 // (an empty slot holds the row itself)
                ++deg[(size_t)i];
                const size_t b = (size_t)deg[(size_t)j]++ * npad + (size_t)j;
                const bool at_j = own[(size_t)j] < own[(size_t)i];
                const int32_t o = at_j ? j : (int32_t)i, q = at_j ? (int32_t)i : j;
                const size_t c = (size_t)own[(size_t)o]++ * npad + (size_t)o;
                if (b >= rsz || c >= esz || ri[b] != (int32_t)i || ei[c] != q)
                    return set_err(ctx, LFPSQP_ERR_ARG, "sphess_map: the handle's two forms do not describe one pattern (row %lld)", (long long)i);
                rs[b] = rs[a];
                es[c] = rs[a];
            }
        }
    }
    lfpsqp_sphess_map* M = new lfpsqp_sphess_map();
    M->n = n; M->nnz = nnz; M->ndiag = ndiag; M->max_dup = max_dup; M->Kr = Kr; M->Ke = Ke; M->npad = S->npad;
    bool ok = true;
    auto dev_copy = [&](int32_t** dst, const std::vector<int32_t>& src) {
        if (!ok) return;
        ok = hipMalloc((void**)dst, src.size() * sizeof(int32_t)) == hipSuccess;
        if (ok) ok = hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    };
    dev_copy(&M->rsrc, rs);
    dev_copy(&M->esrc, es);
    dev_copy(&M->dsrc, ds);
    if (max_dup > 1) dev_copy(&M->next, nx);
    if (ok) ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) {
        lfpsqp_sphess_map_free(ctx, M);
        return set_err(ctx, LFPSQP_ERR_HIP, "sphess_map: device allocation / upload failed");
    }
    if (!S->pattern_refs) S->pattern_refs = new int(1);
    ++*S->pattern_refs;
    M->pattern_refs = S->pattern_refs;
    M->ridx = S->ridx;
    M->eidx = S->eidx;
    *out = M;
    return 0;
}

int lfpsqp_sphess_map_info(const lfpsqp_sphess_map* M, int64_t* nnz, int64_t* ndiag, int64_t* max_dup) {
    if (!M) return LFPSQP_ERR_ARG;
    if (nnz) *nnz = M->nnz;
    if (ndiag) *ndiag = M->ndiag;
    if (max_dup) *max_dup = M->max_dup;
    return 0;
}

int lfpsqp_sphess_set_values(lfpsqp_ctx* ctx, const lfpsqp_sphess_map* M, const lfpsqp_vec* vals, lfpsqp_vec* diag, lfpsqp_sphess* H) {
    LF_ARG(ctx, ctx && M && vals && vals->n >= M->nnz);
    LF_ARG(ctx, !diag || (diag->n >= M->n && diag->p != vals->p));
    LF_ARG(ctx, !H || (H->ridx == M->ridx && H->eidx == M->eidx));          // any handle on the map's pattern
    if (ctx->comm_active())
        return set_err(ctx, LFPSQP_ERR_UNSUPPORTED, "lfpsqp_sphess_set_values: one rank only (no halo exchange between row shards)");
    if (M->n == 0 || !(diag || H)) return 0;
    double* dp = diag ? diag->p : nullptr;
    if (M->next) return set_values_launch<true>(ctx, M, vals->p, dp, H);
    return set_values_launch<false>(ctx, M, vals->p, dp, H);
}

}  // extern "C"
