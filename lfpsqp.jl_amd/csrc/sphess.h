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

}  // namespace lfpsqp
