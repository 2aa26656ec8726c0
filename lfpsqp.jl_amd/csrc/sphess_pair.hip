// lfpsqp_sphess_pair_eval: a PAIR potential between points of dim = 2 or 3 unknowns each,  scale * sum_e w_e psi(x_p - x_q)  over the point edges of
// a handle made by lfpsqp_sphess_create_points (unknown dim*p + c = component c of point p) -- its value, its gradient, the diagonal and the values of
// both ELL forms of a second handle on the same pattern, as lfpsqp_sphess_edge_eval does for one unknown per vertex (sphess_edge.hip).
// With t = x_p - x_q, q = |t|^2:  grad psi = a t,  the Hessian block  B = a I + b (t t'):
//   kind 0: psi = q/2                                 a = 1          b = 0
//   kind 1: psi = (r - l)^2 / 2,  r = sqrt(q)         a = 1 - l/r    b = l / (r q)                         (a spring of rest length l = delta)
//   kind 2: psi = q / (s + 1),  s = sqrt(1 + q/d^2)   a = 1/s        b = -(1/d^2) / (s (1 + q/d^2))        (radial pseudo-Huber, d = delta)
// Stored values: -(scale w)(a [c == c'] + b (t_c t_c')) at ((p,c),(q,c')), scale * sum_q w_pq b (t_c t_c') at the intra-point entry ((p,c),(p,c')).
//
// LANES OWN SCALAR ROWS, two per lane (i, i + 1), as every functor of sphess_edge.hip: the ELL arrays are laid out by scalar row, so the index,
// weight and value of a slot are one aligned 8 / 16 / 16-byte access per lane and consecutive lanes are coalesced, run_vec and its pad-row rule apply
// unchanged, and grad / diag are one 16-byte read-modify-write.  In 2-D the pair (i, i + 1) IS a point, in 3-D it is not; either way each row runs its
// own walk, so the square root and the division of a neighbour are computed once per ROW, dim times per point.  The other choice, a lane per point
// (dim rows of dim*deg + dim - 1 slots: strided 8-byte accesses in 3-D, dim times the registers, a launcher of its own) is not built: FINDINGS.md 23.
//
// A row's slots are in increasing index order, so the dim slots of a neighbour q are consecutive and start at its component 0: (a, b) and t are
// computed at that slot and kept for the next dim - 1.  The slots of the point itself (dim - 1 of them, between the lower and the higher neighbours)
// are written after the walk from their sums; an empty slot holds the row itself and is left alone.  Rows >= dim*npoints (a slack row) and the pad
// row behind an odd n have no couplings and are skipped.
// BITS.  t_c t_c' is formed first and multiplied by b afterwards; (-t_c)(-t_c') and commutativity give the row (q,c') the bits of the row (p,c); q is
// an fma chain over the components in order (even in t); both rows of an intra-point pair walk the same neighbours in the same order.  The edge
// form recomputes a cross-point entry from its owner's side with the same expressions, and COPIES an intra-point entry from the row form of H that
// the row kernel has just written (found by searching the owner's row for the partner).  Every fma is written out: no contraction is relied on.
// ROUNDINGS per value (a count k stands for gamma_k; t_c = fl(x_pc - x_qc) 1, against the exact difference; tests/test_sphess_pair.py holds the
// kernels to these), cq = dim + 2 for q (t_c^2 carries 3, each further fma one more):
//   kind 1: r = sqrt(q): cr = ceil(cq / 2) + 1 = 3 / 4 (2-D / 3-D).  psi = ((r - l)(r - l)) / 2: 2 cr + 3 = 9 / 11 on (r + l)^2 / 2.  a = 1 - l/r: cr + 2 =
//           5 / 6 on 1 + l/r.  b = l / (r q): cr + cq + 2 = 9 / 11.
//   kind 2 (1/d^2 on the host: 2): u = fma(q, 1/d^2, 1): cq + 3 = 7 / 8.  s = sqrt(u): ceil((cq + 3) / 2) + 1 = 5.  psi = q / (s + 1): cq + 7 = 11 / 12.
//           a = 1/s: 6.  b = -(1/d^2) / (s u): 2 + (5 + cq + 3 + 1) + 1 = cq + 12 = 16 / 17.
//   v = a [c == c'] + b (t_c t_c') (one fma, or one product; t_c t_c' carries 3): cv = count(b) + 4 = 13 / 15 (kind 1) and 20 / 21 (kind 2), on
//           |a|-terms [c == c'] + |b t_c t_c'|, the |a|-terms being 1 + l/r (kind 1) and a (kind 2).
//   a stored cross-point value: fl(scale w) and the product: cv + 2.  grad term a t_c: count(a) + 2.
//   a row sum (grad, diag, an intra-point entry): at most deg additions of the fma chain (one per neighbour) and one rounding with scale:
//           deg + count(a) + 3 (grad), deg + cv + 1 (diag, intra-point).   f: as in sphess_edge.hip, npoints deg + count(psi) + 1.
//   lfpsqp_sphess_pair_eval_ex (below: a parameter per edge, anchors): a per-edge l / d is an exact input and 1/d^2 costs the same 2 on the device;
//           an anchor's t_c = fl(x_pc - a_c) is 1, its (psi, a, b, v) the neighbour's, and it adds one fma to each chain of its row: deg becomes
//           D = the largest (neighbours + anchors) of a point in the three row-sum counts and in f's (tests/test_sphess_pair_ex.py).
#include <math.h>

#include "sphess.h"

namespace lfpsqp {

template <int KIND>
struct PairPot {
    double delta;              // l (kind 1)
    double rd2;                // 1 / delta^2 (kind 2)
    // (psi, a, b) at q = |t|^2
    __device__ __forceinline__ void eval(double q, double& psi, double& a, double& b) const {
        if (KIND == 0) {
            psi = 0.5 * q; a = 1.0; b = 0.0;
        } else if (KIND == 1) {
            const double r = sqrt(q), e = r - delta;
            psi = 0.5 * (e * e); a = 1.0 - delta / r; b = delta / (r * q);
        } else {
            const double u = fma(q, rd2, 1.0), s = sqrt(u);
            psi = q / (s + 1.0); a = 1.0 / s; b = -(rd2 / (s * u));
        }
    }
};

__device__ __forceinline__ double sel(bool c, double a, double b) { return c ? a : b; }

template <int DIM>
__device__ __forceinline__ double pick(int c, double t0, double t1, double t2) {
    return c == 0 ? t0 : (DIM == 2 || c == 1) ? t1 : t2;
}

// t = x_p - x_q for the neighbour point at index j0 (its component 0) and q = |t|^2
template <int DIM>
__device__ __forceinline__ double diff(const double* x, double xp0, double xp1, double xp2, int32_t j0, double& t0, double& t1, double& t2) {
    t0 = xp0 - x[j0];
    t1 = xp1 - x[j0 + 1];
    double q = fma(t1, t1, t0 * t0);
    if (DIM == 3) { t2 = xp2 - x[j0 + 2]; q = fma(t2, t2, q); }
    else t2 = 0.0;
    return q;
}

// One scalar row's walk over its slots (row form).  The state is named, not indexed: no array that the compiler could put into scratch.
template <int DIM, int KIND, bool WF, bool WV>
struct PairRow {
    int32_t r;                 // the row, dim*p + c
    int32_t base;              // dim*p
    int c;
    bool on;                   // a row of a point (not a slack row, not a pad row)
    double xp0, xp1, xp2;
    double t0, t1, t2, tc, a, b;
    double e, g, d, m0, m1;
    int kin;                   // the first slot of the point itself; -1: not met yet

    __device__ __forceinline__ void init(int64_t row, bool valid, int64_t nrows, const double* x) {
        on = valid && row < nrows;
        r = (int32_t)row;
        const int32_t p = r / DIM;
        base = p * DIM;
        c = r - base;
        xp0 = xp1 = xp2 = 0.0;
        if (on) {
            xp0 = x[base]; xp1 = x[base + 1];
            if (DIM == 3) xp2 = x[base + 2];
        }
        t0 = t1 = t2 = tc = a = b = 0.0;
        e = g = d = m0 = m1 = 0.0;
        kin = -1;
    }
    // slot k holding (j, w): true and the new value in h when the slot is a cross-point entry; pot: PairPot<KIND>, or PairPotAt<KIND> (below)
    template <class POT>
    __device__ __forceinline__ bool slot(const POT& pot, const double* x, double scale, int k, int32_t j, double w, double& h) {
        if (!on) return false;
        const int32_t jb = (j / DIM) * DIM;
        if (jb == base) {                           // the row itself (an empty slot) or another component of its point
            if (j != r && kin < 0) kin = k;
            return false;
        }
        const int cc = j - jb;
        if (cc == 0) {
            const double q = diff<DIM>(x, xp0, xp1, xp2, j, t0, t1, t2);
            double psi;
            pot.eval(q, psi, a, b);
            tc = pick<DIM>(c, t0, t1, t2);
            if (WF && c == 0) e = fma(w, psi, e);   // (the point's energy, once: at its component 0)
            if (WV) g = fma(w, a * tc, g);
        }
        double v;
        if (KIND == 0) v = cc == c ? 1.0 : 0.0;
        else {
            const double tt = tc * pick<DIM>(cc, t0, t1, t2);
            v = cc == c ? fma(b, tt, a) : b * tt;
        }
        if (WV) {
            // one fma into d (cc == c) or into the sum of the point's other components, in increasing order m0, m1 -- selected BY VALUE (sel: its
            // arguments are loaded first).  Three conditional updates, or ?: between the members themselves (an lvalue), become one update through a
            // pointer into this object, and the object then lives in scratch.
            const int k3 = cc == c ? 0 : (DIM == 2 || cc == (c == 0 ? 1 : 0)) ? 1 : 2;
            const double s = fma(w, v, sel(k3 == 0, d, sel(k3 == 1, m0, m1)));
            d = sel(k3 == 0, s, d);
            m0 = sel(k3 == 1, s, m0);
            m1 = sel(k3 == 2, s, m1);
        }
        h = KIND == 0 && cc != c ? 0.0 : -((scale * w) * v);
        return true;
    }
    // the intra-point slots, from their sums
    __device__ __forceinline__ void intra(double scale, double* hval, int64_t npad) const {
        if (!on || kin < 0) return;
        double* hp = hval + (int64_t)kin * npad + r;
        hp[0] = KIND == 0 ? 0.0 : scale * m0;
        if (DIM == 3) hp[npad] = KIND == 0 ? 0.0 : scale * m1;
    }
};

// Row form, two rows per lane.  WF: the energy goes to the reduction (every point edge is seen from both ends, at component 0 of either: the host
// halves the sum); WV: grad / diag / hval, each optional.  <WF, !WV> writes nothing.  The slot loop is rolled for every kind, as the scalar kinds
// 1 and 2 (FINDINGS.md 23 has the resource report).
template <bool WF, bool WV, int DIM, int KIND>
struct PairRowF {
    PairPot<KIND> pot;
    const int32_t* idx;
    const double* w;
    int64_t npad;
    int K;
    int64_t nrows;             // dim * npoints
    const double* x;
    double scale;
    double* grad;
    double* diag;
    double* hval;
    __device__ __forceinline__ bool skip() const { return false; }
    __device__ __forceinline__ void apply(int64_t i, bool v0, bool v1, double* red) const {
        if (!v0 || i >= nrows) return;
        PairRow<DIM, KIND, WF, WV> r0, r1;
        r0.init(i, v0, nrows, x);
        r1.init(i + 1, v1, nrows, x);
        const int32_t* ip = idx + i;
        const double* wp = w + i;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int64_t o = (int64_t)k * npad;
            const int2 jj = *reinterpret_cast<const int2*>(ip + o);
            const double2 ww = ld2(wp + o);
            double h0 = 0.0, h1 = 0.0;
            const bool s0 = r0.slot(pot, x, scale, k, jj.x, ww.x, h0);
            const bool s1 = r1.slot(pot, x, scale, k, jj.y, ww.y, h1);
            if (WV && hval) store_rows(hval, i, o, s0, s1, h0, h1);
        }
        if (WF) red[0] += r0.e + r1.e;
        if (WV) {
            if (hval) { r0.intra(scale, hval, npad); r1.intra(scale, hval, npad); }
            if (grad) add_rows(grad, i, r1.on, scale, r0.g, r1.g);
            if (diag) add_rows(diag, i, r1.on, scale, r0.d, r1.d);
        }
    }
};

// One slot of the edge form at owner row `row`: partner j, weight w.  A cross-point entry is the row kernel's expression from the owner's side; an
// intra-point entry is copied from the owner's row of H's row form (at most dim - 1 such slots in a row; the row kernel ran before).
template <int DIM, int KIND, class POT>
__device__ __forceinline__ bool pair_own_slot(const POT& pot, const double* x, double scale, const int32_t* ridx, const double* hrow, int64_t npad,
                                              int Kr, int64_t row, bool valid, int64_t nrows, int32_t j, double w, double& h) {
    if (!valid || row >= nrows) return false;
    const int32_t r = (int32_t)row, base = (r / DIM) * DIM, jb = (j / DIM) * DIM;
    if (jb == base) {
        if (j == r) return false;                   // an empty slot
        h = 0.0;
#pragma unroll 1
        for (int k = 0; k < Kr; ++k)
            if (ridx[(int64_t)k * npad + r] == j) { h = hrow[(int64_t)k * npad + r]; break; }
        return true;
    }
    const int c = r - base, cc = j - jb;
    if (KIND == 0) {
        h = cc == c ? -(scale * w) : 0.0;
        return true;
    }
    double t0, t1, t2, psi, a, b;
    const double q = diff<DIM>(x, x[base], x[base + 1], DIM == 3 ? x[base + 2] : 0.0, jb, t0, t1, t2);
    pot.eval(q, psi, a, b);
    const double tt = pick<DIM>(c, t0, t1, t2) * pick<DIM>(cc, t0, t1, t2);
    const double v = cc == c ? fma(b, tt, a) : b * tt;
    h = -((scale * w) * v);
    return true;
}

template <int DIM, int KIND>
struct PairOwnF {
    PairPot<KIND> pot;
    const int32_t* idx;        // the edge form
    const double* w;
    int64_t npad;
    int K;
    const int32_t* ridx;       // the row form: the pattern, and H's values
    const double* hrow;
    int Kr;
    int64_t nrows;
    const double* x;
    double scale;
    double* hval;
    __device__ __forceinline__ bool skip() const { return false; }
    __device__ __forceinline__ void apply(int64_t i, bool v0, bool v1, double*) const {
        if (!v0 || i >= nrows) return;
        const int32_t* ip = idx + i;
        const double* wp = w + i;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int64_t o = (int64_t)k * npad;
            const int2 jj = *reinterpret_cast<const int2*>(ip + o);
            const double2 ww = ld2(wp + o);
            double h0 = 0.0, h1 = 0.0;
            const bool s0 = pair_own_slot<DIM, KIND>(pot, x, scale, ridx, hrow, npad, Kr, i, v0, nrows, jj.x, ww.x, h0);
            const bool s1 = pair_own_slot<DIM, KIND>(pot, x, scale, ridx, hrow, npad, Kr, i + 1, v1, nrows, jj.y, ww.y, h1);
            store_rows(hval, i, o, s0, s1, h0, h1);
        }
    }
};

// ---- lfpsqp_sphess_pair_eval_ex: a parameter per edge (one more value stream on the pattern: the handle P) and anchors (lfpsqp_anchors) --------
// The functors above keep their code; these two have their shape and go through the same PairRow::slot / pair_own_slot, with the potential of the
// slot's own parameter.  "Has P" and "has anchors" are wave-uniform RUN-TIME tests (a null pointer, a width of 0), not template flags: four times
// the 18 row kernels would buy nothing the resource report shows (FINDINGS.md 25: no scratch, the VGPRs of PairRowF + at most 14).
// ROUNDINGS.  A per-edge l_e / delta_e is an exact input, as delta is, and 1/delta_e^2 = 1.0 / (delta_e delta_e) is the host's expression: every
// count of the head of this file stands.  An anchor's t_c = fl(x_pc - a_c) is one rounding, (psi, a, b) and v are the neighbour's expressions, and
// it adds one fma to each of the row's chains: with ka the most anchors on a point, deg becomes deg + ka in the counts of grad, diag and the
// intra-point entry, and npoints deg becomes npoints (deg + ka) in f's (the factor 2 u of an anchor's energy term is exact).

// The potential with the parameter of ONE slot; uni: the parameter is the call's delta and rd2 its 1 / delta^2 from the host (wave-uniform)
template <int KIND>
struct PairPotAt {
    double par;
    double rd2;
    bool uni;
    __device__ __forceinline__ void eval(double q, double& psi, double& a, double& b) const {
        const PairPot<KIND> pot{par, KIND == 2 ? (uni ? rd2 : 1.0 / (par * par)) : 0.0};
        pot.eval(q, psi, a, b);
    }
};

// One anchor slot of a row, after its neighbours: weight u (0.0: an empty slot, skipped before anything else is loaded), position pos[base ..
// base + dim - 1], parameter par[row] or the call's delta.  The sums take the terms PairRow::slot gives them for a neighbour at pos, in the same
// expressions; the energy is counted at component 0 with 2 u (exact), because eval_finish halves the sum.  No entry between points is written.
template <int DIM, int KIND, bool WF, bool WV>
__device__ __forceinline__ void pair_anchor(PairRow<DIM, KIND, WF, WV>& r, const PairPot<KIND>& uni, const double* pos, const double* par, double u) {
    if (!r.on || u == 0.0) return;
    double t0, t1, t2, psi, a, b;
    const double q = diff<DIM>(pos, r.xp0, r.xp1, r.xp2, r.base, t0, t1, t2);
    const PairPotAt<KIND> pot{KIND != 0 && par ? par[r.r] : uni.delta, uni.rd2, !par};
    pot.eval(q, psi, a, b);
    const double tc = pick<DIM>(r.c, t0, t1, t2);
    if (WF && r.c == 0) r.e = fma(u + u, psi, r.e);
    if (WV) {
        r.g = fma(u, a * tc, r.g);
        if (KIND == 0) r.d = fma(u, 1.0, r.d);
        else {
            // the point's other components in increasing order, as slot() meets them: m0, then m1
            r.d = fma(u, fma(b, tc * tc, a), r.d);
            r.m0 = fma(u, b * (tc * pick<DIM>(r.c == 0 ? 1 : 0, t0, t1, t2)), r.m0);
            if (DIM == 3) r.m1 = fma(u, b * (tc * pick<DIM>(r.c == 2 ? 1 : 2, t0, t1, t2)), r.m1);
        }
    }
}

template <bool WF, bool WV, int DIM, int KIND>
struct PairRowExF {
    PairPot<KIND> pot;         // the call's delta: the edges' parameter without pval, the anchors' without apar
    const int32_t* idx;
    const double* w;
    const double* pval;        // P's row form, or nullptr
    int64_t npad;
    int K;
    int64_t nrows;             // dim * npoints
    const double* x;
    double scale;
    const double* apos;        // the anchors: aw slots of npad entries each
    const double* au;
    const double* apar;        // or nullptr
    int aw;
    double* grad;
    double* diag;
    double* hval;
    __device__ __forceinline__ bool skip() const { return false; }
    __device__ __forceinline__ void apply(int64_t i, bool v0, bool v1, double* red) const {
        if (!v0 || i >= nrows) return;
        PairRow<DIM, KIND, WF, WV> r0, r1;
        r0.init(i, v0, nrows, x);
        r1.init(i + 1, v1, nrows, x);
        const int32_t* ip = idx + i;
        const double* wp = w + i;
        const bool uni = KIND == 0 || !pval;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int64_t o = (int64_t)k * npad;
            const int2 jj = *reinterpret_cast<const int2*>(ip + o);
            const double2 ww = ld2(wp + o);
            const double2 pp = uni ? make_double2(pot.delta, pot.delta) : ld2(pval + i + o);
            double h0 = 0.0, h1 = 0.0;
            const bool s0 = r0.slot(PairPotAt<KIND>{pp.x, pot.rd2, uni}, x, scale, k, jj.x, ww.x, h0);
            const bool s1 = r1.slot(PairPotAt<KIND>{pp.y, pot.rd2, uni}, x, scale, k, jj.y, ww.y, h1);
            if (WV && hval) store_rows(hval, i, o, s0, s1, h0, h1);
        }
#pragma unroll 1
        for (int k = 0; k < aw; ++k) {
            const int64_t o = (int64_t)k * npad;
            const double2 uu = ld2(au + i + o);
            const double* pk = apar ? apar + o : nullptr;
            pair_anchor(r0, pot, apos + o, pk, uu.x);
            pair_anchor(r1, pot, apos + o, pk, uu.y);
        }
        if (WF) red[0] += r0.e + r1.e;
        if (WV) {
            if (hval) { r0.intra(scale, hval, npad); r1.intra(scale, hval, npad); }
            if (grad) add_rows(grad, i, r1.on, scale, r0.g, r1.g);
            if (diag) add_rows(diag, i, r1.on, scale, r0.d, r1.d);
        }
    }
};

// The edge form with P's edge form beside it: the two forms of P hold the same bits, so both sides evaluate (psi, a, b) from identical inputs.
template <int DIM, int KIND>
struct PairOwnExF {
    const int32_t* idx;        // the edge form
    const double* w;
    const double* pval;        // P's edge form
    int64_t npad;
    int K;
    const int32_t* ridx;       // the row form: the pattern, and H's values
    const double* hrow;
    int Kr;
    int64_t nrows;
    const double* x;
    double scale;
    double* hval;
    __device__ __forceinline__ bool skip() const { return false; }
    __device__ __forceinline__ void apply(int64_t i, bool v0, bool v1, double*) const {
        if (!v0 || i >= nrows) return;
        const int32_t* ip = idx + i;
        const double* wp = w + i;
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int64_t o = (int64_t)k * npad;
            const int2 jj = *reinterpret_cast<const int2*>(ip + o);
            const double2 ww = ld2(wp + o);
            const double2 pp = ld2(pval + i + o);
            double h0 = 0.0, h1 = 0.0;
            const bool s0 = pair_own_slot<DIM, KIND>(PairPotAt<KIND>{pp.x, 0.0, false}, x, scale, ridx, hrow, npad, Kr, i, v0, nrows, jj.x, ww.x, h0);
            const bool s1 = pair_own_slot<DIM, KIND>(PairPotAt<KIND>{pp.y, 0.0, false}, x, scale, ridx, hrow, npad, Kr, i + 1, v1, nrows, jj.y, ww.y, h1);
            store_rows(hval, i, o, s0, s1, h0, h1);
        }
    }
};

template <int DIM, int KIND>
static int pair_eval_ex_kind(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, double delta, double rd2, const lfpsqp_sphess* P, const lfpsqp_anchors* A, double scale,
                             const double* x, bool wantf, double* grad, double* diag, lfpsqp_sphess* H) {
    const PairPot<KIND> pot{delta, rd2};
    const int64_t nrows = (int64_t)DIM * W->pts.npoints;
    const double* hr = H ? H->rval : nullptr;
    double* he = H ? H->eval : nullptr;
    auto launch = [&](const auto& own) {
        return eval_launch<PairRowExF, DIM, KIND>(ctx, W, wantf, grad, diag, H, own, pot, W->ridx, W->rval, P ? P->rval : nullptr, W->npad, W->Kr, nrows, x,
                                                  scale, A ? A->pos : nullptr, A ? A->u : nullptr, A ? A->par : nullptr, A ? A->width : 0);
    };
    if constexpr (KIND != 0) {
        if (P) return launch(PairOwnExF<DIM, KIND>{W->eidx, W->eval, P->eval, W->npad, W->Ke, W->ridx, hr, W->Kr, nrows, x, scale, he});
    }
    // (the anchors write no entry between points: without P the edge form is the uniform call's)
    return launch(PairOwnF<DIM, KIND>{pot, W->eidx, W->eval, W->npad, W->Ke, W->ridx, hr, W->Kr, nrows, x, scale, he});
}

template <int DIM>
static int pair_eval_ex_dim(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, int kind, double delta, double rd2, const lfpsqp_sphess* P, const lfpsqp_anchors* A,
                            double scale, const double* x, bool wantf, double* grad, double* diag, lfpsqp_sphess* H) {
    if (kind == 0) return pair_eval_ex_kind<DIM, 0>(ctx, W, delta, rd2, P, A, scale, x, wantf, grad, diag, H);
    if (kind == 1) return pair_eval_ex_kind<DIM, 1>(ctx, W, delta, rd2, P, A, scale, x, wantf, grad, diag, H);
    return pair_eval_ex_kind<DIM, 2>(ctx, W, delta, rd2, P, A, scale, x, wantf, grad, diag, H);
}

template <int DIM, int KIND>
static int pair_eval_kind(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, double delta, double rd2, double scale, const double* x, bool wantf, double* grad,
                          double* diag, lfpsqp_sphess* H) {
    const PairPot<KIND> pot{delta, rd2};
    const int64_t nrows = (int64_t)DIM * W->pts.npoints;
    return eval_launch<PairRowF, DIM, KIND>(
        ctx, W, wantf, grad, diag, H,
        PairOwnF<DIM, KIND>{pot, W->eidx, W->eval, W->npad, W->Ke, W->ridx, H ? H->rval : nullptr, W->Kr, nrows, x, scale, H ? H->eval : nullptr},
        pot, W->ridx, W->rval, W->npad, W->Kr, nrows, x, scale);
}

template <int DIM>
static int pair_eval_dim(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, int kind, double delta, double rd2, double scale, const double* x, bool wantf,
                         double* grad, double* diag, lfpsqp_sphess* H) {
    if (kind == 0) return pair_eval_kind<DIM, 0>(ctx, W, delta, rd2, scale, x, wantf, grad, diag, H);
    if (kind == 1) return pair_eval_kind<DIM, 1>(ctx, W, delta, rd2, scale, x, wantf, grad, diag, H);
    return pair_eval_kind<DIM, 2>(ctx, W, delta, rd2, scale, x, wantf, grad, diag, H);
}

}  // namespace lfpsqp

using namespace lfpsqp;

extern "C" int lfpsqp_sphess_pair_eval(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, int kind, double delta, double scale, const lfpsqp_vec* x, double* f,
                                       lfpsqp_vec* grad, lfpsqp_vec* diag, lfpsqp_sphess* H) {
    LF_ARG(ctx, ctx && W && x && kind >= 0 && kind <= 2 && std::isfinite(scale));
    LF_ARG(ctx, W->pts.dim == 2 || W->pts.dim == 3);             // a handle of lfpsqp_sphess_create_points (or a handle on its pattern)
    const int64_t nrows = (int64_t)W->pts.dim * W->pts.npoints;
    LF_ARG(ctx, kind != 1 || (std::isfinite(delta) && delta >= 0.0));
    LF_ARG(ctx, kind != 2 || (std::isfinite(delta) && delta > 0.0));
    LF_TRY(eval_check(ctx, "lfpsqp_sphess_pair_eval", W, nrows, x, f, grad, diag, H));
    if (nrows == 0 || !(f || grad || diag || H)) return 0;
    const double rd2 = kind == 2 ? 1.0 / (delta * delta) : 0.0;
    double *gp = grad ? grad->p : nullptr, *dp = diag ? diag->p : nullptr;
    if (W->pts.dim == 2) LF_TRY(pair_eval_dim<2>(ctx, W, kind, delta, rd2, scale, x->p, f != nullptr, gp, dp, H));
    else LF_TRY(pair_eval_dim<3>(ctx, W, kind, delta, rd2, scale, x->p, f != nullptr, gp, dp, H));
    return eval_finish(ctx, scale, f);
}

extern "C" int lfpsqp_sphess_pair_eval_ex(lfpsqp_ctx* ctx, const lfpsqp_sphess* W, int kind, double delta, const lfpsqp_sphess* P, const lfpsqp_anchors* A,
                                          double scale, const lfpsqp_vec* x, double* f, lfpsqp_vec* grad, lfpsqp_vec* diag, lfpsqp_sphess* H) {
    if (!P && !A) return lfpsqp_sphess_pair_eval(ctx, W, kind, delta, scale, x, f, grad, diag, H);
    LF_ARG(ctx, ctx && W && x && kind >= 0 && kind <= 2 && std::isfinite(scale));
    LF_ARG(ctx, W->pts.dim == 2 || W->pts.dim == 3);
    const int64_t nrows = (int64_t)W->pts.dim * W->pts.npoints;
    LF_ARG(ctx, !P || (kind != 0 && P != H && P->ridx == W->ridx && P->eidx == W->eidx));     // a handle on W's pattern; kind 0 has no parameter
    LF_ARG(ctx, !A || (A->n == W->n && A->npoints == W->pts.npoints && A->dim == W->pts.dim && A->npad == W->npad));
    const bool uses_delta = !P || (A && !A->par);
    LF_ARG(ctx, !uses_delta || kind != 1 || (std::isfinite(delta) && delta >= 0.0));
    LF_ARG(ctx, !uses_delta || kind != 2 || (std::isfinite(delta) && delta > 0.0));
    LF_TRY(eval_check(ctx, "lfpsqp_sphess_pair_eval_ex", W, nrows, x, f, grad, diag, H));
    if (nrows == 0 || !(f || grad || diag || H)) return 0;
    const double rd2 = kind == 2 && uses_delta ? 1.0 / (delta * delta) : 0.0;
    double *gp = grad ? grad->p : nullptr, *dp = diag ? diag->p : nullptr;
    if (W->pts.dim == 2) LF_TRY(pair_eval_ex_dim<2>(ctx, W, kind, delta, rd2, P, A, scale, x->p, f != nullptr, gp, dp, H));
    else LF_TRY(pair_eval_ex_dim<3>(ctx, W, kind, delta, rd2, P, A, scale, x->p, f != nullptr, gp, dp, H));
    return eval_finish(ctx, scale, f);
}
