/* A walk over the scratch-buffer layouts of the library (csrc/internal.h, Layout) for a SANITIZER build of the CPU emulator:
 *     make -C tests/c_consumer asan-walk
 * compiles this file with -fsanitize=address,undefined, links it to tests/emu/_build_asan/liblfpsqp_emu.so and runs it -- an ordinary
 * executable on the CPU, nothing preloaded, never on a GPU, not a pytest test.  It calls the C ABI at the smallest shapes that take each branch of
 * the layouts in ctx->small, d_m / h_m, d_nvec and d_tri (odd row counts: pads and tails are exercised), prints one line per call and exits
 * non-zero on any error status.  It asserts nothing about numbers: the suite does that.  What a clean run proves: no access outside an
 * allocation -- small and d_tri are allocated exactly, so an overrun of those is reported; d_m and d_nvec are rounded up to whole tiles, which
 * hides small overruns; two regions overlapping INSIDE a buffer is not an address error (the suite sees that as wrong numbers). */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lfpsqp_hip.h"

static lfpsqp_ctx* ctx;
static int failed;

/* set-up calls: any error ends the run */
#define CK(call)                                                                       \
    do {                                                                               \
        int rc_ = (call);                                                              \
        if (rc_ != 0) {                                                                \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, lfpsqp_last_error(ctx));     \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)
/* the calls the walk is about: one line each */
#define STEP(what, call)                                                               \
    do {                                                                               \
        int rc_ = (call);                                                              \
        printf("%-74s %s\n", what, rc_ == 0 ? "ok" : "ERROR");                         \
        fflush(stdout);                                                                \
        if (rc_ != 0) {                                                                \
            fprintf(stderr, "  status %d: %s\n", rc_, lfpsqp_last_error(ctx));         \
            failed = 1;                                                                \
        }                                                                              \
    } while (0)

/* everything allocated is kept in pools and released at the end */
enum { POOL = 16384 };
static lfpsqp_vec* vpool[POOL];
static lfpsqp_mat* mpool[POOL];
static void* hpool[POOL];
static lfpsqp_spmat* sppool[64];
static lfpsqp_sphess* shpool[64];
static int nv_, nm_, nh_, nsp_, nsh_;

static lfpsqp_vec* vec(int64_t n) {
    lfpsqp_vec* v = NULL;
    CK(lfpsqp_vec_alloc(ctx, n, &v));
    if (nv_ == POOL) exit(3);
    return vpool[nv_++] = v;
}
static lfpsqp_vec* vec_fill(int64_t n, double value) {
    lfpsqp_vec* v = vec(n);
    CK(lfpsqp_vec_fill(ctx, v, value));
    return v;
}
static lfpsqp_vec* vec_hash(int64_t n, uint64_t seed, double scale, double shift) {
    lfpsqp_vec* v = vec(n);
    CK(lfpsqp_vec_hash_fill(ctx, v, seed, 0, scale, shift));
    return v;
}
/* a stacked vector [x | gap | y] with both halves filled, the gap left zero */
static lfpsqp_vec* stacked_hash(int64_t N, uint64_t seed, double scale, double shift) {
    const int64_t hs = lfpsqp_half_stride(N);
    lfpsqp_vec* v = vec(hs + N);
    CK(lfpsqp_vec_copy_range(ctx, v, 0, vec_hash(N, seed, scale, shift), 0, N));
    CK(lfpsqp_vec_copy_range(ctx, v, hs, vec_hash(N, seed + 100, scale, shift), 0, N));
    return v;
}
static lfpsqp_mat* mat(int64_t n, int64_t m) {
    lfpsqp_mat* M = NULL;
    CK(lfpsqp_mat_alloc(ctx, n, m, &M));
    if (nm_ == POOL) exit(3);
    return mpool[nm_++] = M;
}
static lfpsqp_mat* mat_hash(int64_t n, int64_t m, uint64_t seed, double scale) {
    lfpsqp_mat* M = mat(n, m);
    CK(lfpsqp_mat_hash_fill(ctx, M, seed, 0, n, scale, n, m));
    return M;
}
static void* host(size_t bytes) {
    void* p = calloc(bytes ? bytes : 1, 1);
    if (!p || nh_ == POOL) exit(3);
    return hpool[nh_++] = p;
}
static double* hostd(int64_t count) { return (double*)host(sizeof(double) * (size_t)count); }
static double unit(uint64_t k) { /* a cheap deterministic value in [-1, 1) */
    k = (k ^ (k >> 30)) * 0xbf58476d1ce4e5b9ULL;
    k = (k ^ (k >> 27)) * 0x94d049bb133111ebULL;
    return (double)((k ^ (k >> 31)) >> 11) / 4503599627370496.0 - 1.0;
}

/* the bound manifolds of N variables at a point inside the box */
typedef struct {
    int64_t N, hs, nv;
    lfpsqp_vec *q, *r, *s, *t, *xaug, *Dx, *Dy, *S, *sx, *sy;
    lfpsqp_ineq_data id;
} bounds;
static bounds make_bounds(int64_t N) {
    bounds b;
    b.N = N; b.hs = lfpsqp_half_stride(N); b.nv = b.hs + N;
    b.q = vec(N); b.r = vec(N); b.s = vec(N); b.t = vec(N);
    CK(lfpsqp_ineq_data_build(ctx, vec_fill(N, -1.5), vec_fill(N, 2.0), b.q, b.r, b.s, b.t));
    b.id.q = b.q; b.id.r = b.r; b.id.s = b.s; b.id.t = b.t; b.id.n = N;
    b.xaug = vec(b.nv);
    CK(lfpsqp_vec_copy_range(ctx, b.xaug, 0, vec_hash(N, 31, 0.3, 0.0), 0, N));
    CK(lfpsqp_generate_initial_y(ctx, b.xaug, &b.id));
    b.Dx = vec(N); b.Dy = vec(N); b.S = vec(N); b.sx = vec(N); b.sy = vec(N);
    CK(lfpsqp_inequality_gradient(ctx, b.xaug, &b.id, b.Dx, b.Dy, b.S, b.sx, b.sy));
    return b;
}

/* the factors of a constraint-gradient block */
typedef struct {
    int64_t n, m, rank;
    lfpsqp_mat *J, *Z;
    double *Sigma, *Vt, *W;
} factors;
static factors factorize(const char* what, lfpsqp_mat* J, int64_t n, int64_t m, const lfpsqp_vec* w2, int want_Z) {
    factors f;
    f.n = n; f.m = m; f.rank = 0; f.J = J;
    f.Z = want_Z ? mat(n, m) : NULL;
    f.Sigma = hostd(m); f.Vt = hostd(m * m); f.W = hostd(m * m);
    STEP(what, lfpsqp_factorize(ctx, J, w2, f.Z, f.Sigma, f.Vt, f.W, &f.rank, 1e-10));
    return f;
}
/* bases over those factors: materialised, with the generator, in factored form; b != NULL: stacked */
static lfpsqp_basis basis(const factors* f, const bounds* b, int with_Z, int with_gen, const lfpsqp_spmat* SA) {
    lfpsqp_basis U;
    memset(&U, 0, sizeof U);
    U.Z = with_Z ? f->Z : NULL;
    U.ncols = f->rank;
    if (b) { U.Dx = b->Dx; U.Dy = b->Dy; U.sx = b->sx; U.sy = b->sy; }
    if (with_gen) { U.A = f->J; U.W = f->W; }
    U.SA = SA;
    return U;
}
static lfpsqp_projcg_work work(int64_t nv, int64_t m) {
    lfpsqp_projcg_work w;
    w.g = vec(nv); w.d = vec(nv); w.rp = vec(nv); w.Utr = vec(4 * m + 16);
    return w;
}

/* a sparse n x m block with two nonzeros per row, and its dense twin with `extra` dense columns behind it */
static lfpsqp_spmat* sparse_block(int64_t n, int64_t m) {
    int64_t* rows = (int64_t*)host(sizeof(int64_t) * 2 * (size_t)n);
    int64_t* cols = (int64_t*)host(sizeof(int64_t) * 2 * (size_t)n);
    double* vals = hostd(2 * n);
    for (int64_t i = 0; i < n; ++i) {
        rows[2 * i] = rows[2 * i + 1] = i;
        cols[2 * i] = i % m;
        cols[2 * i + 1] = (i % m + 1 + (i / m) % (m - 1)) % m;
        vals[2 * i] = 1.0 + 0.5 * unit((uint64_t)i);
        vals[2 * i + 1] = 0.7 * unit((uint64_t)(i + 100000));
    }
    lfpsqp_spmat* S = NULL;
    CK(lfpsqp_spmat_create(ctx, n, m, 2 * n, rows, cols, vals, &S));
    return sppool[nsp_++] = S;
}
static lfpsqp_mat* dense_twin(const lfpsqp_spmat* S, int64_t n, int64_t m, int64_t extra) {
    lfpsqp_mat* A = mat(n, m + extra);
    CK(lfpsqp_spmat_to_dense(ctx, S, A));
    if (extra > 0) {
        double* col = hostd(n * extra);
        for (int64_t i = 0; i < n * extra; ++i) col[i] = unit((uint64_t)(i + 777777));
        CK(lfpsqp_mat_upload(ctx, A, m, extra, col, n));
    }
    return A;
}

/* ---- lfpsqp_projcg ------------------------------------------------------------------------------------------------------------------ */
static void projcg(const char* what, const lfpsqp_basis* U, const bounds* b, int64_t n, const lfpsqp_vec* c, int64_t maxit, int resume) {
    const int64_t nv = b ? b->nv : n, m = U->ncols;
    lfpsqp_vec* dg = b ? stacked_hash(n, 3, 4.0, 5.0) : vec_hash(n, 3, 4.0, 5.0);
    lfpsqp_vec* rhs = b ? stacked_hash(n, 4, 1.0, 0.0) : vec_hash(n, 4, 1.0, 0.0);
    lfpsqp_vec *x = vec(nv), *lam = vec((b ? n : 0) + m + 1);
    const lfpsqp_diag_op A = {0.0, dg};
    lfpsqp_projcg_work w = work(nv, m);
    int64_t iters = -1;
    double nr = -1.0;
    STEP(what, lfpsqp_projcg(ctx, x, lam, &A, U, rhs, c, 0.0, maxit, b ? 2 * n : n, resume ? 0 : LFPSQP_PROJCG_WANT_LAMBDA, &w, &iters, &nr));
    if (resume)
        STEP("  ... LFPSQP_PROJCG_RESUME after the iteration limit", lfpsqp_projcg(ctx, x, lam, &A, U, rhs, c, 0.0, maxit, b ? 2 * n : n,
                                                                                   LFPSQP_PROJCG_RESUME, &w, &iters, &nr));
}
static void walk_projcg(int64_t n, int64_t nb) {
    char s[160];
    const bounds B = make_bounds(nb);
    /* m = 3: the unfused two-pass path; m = 5: fused */
    lfpsqp_mat* J3 = mat_hash(n, 3, 1, 1.0);
    snprintf(s, sizeof s, "factorize n=%" PRId64 " m=3", n);
    factors f3 = factorize(s, J3, n, 3, NULL, 1);
    lfpsqp_basis U = basis(&f3, NULL, 1, 0, NULL);
    snprintf(s, sizeof s, "projcg n=%" PRId64 " m=3 (two-pass)", n);
    projcg(s, &U, NULL, n, NULL, 6, 0);
    lfpsqp_mat* J5 = mat_hash(n, 5, 1, 1.0);
    snprintf(s, sizeof s, "factorize n=%" PRId64 " m=5", n);
    factors f5 = factorize(s, J5, n, 5, NULL, 1);
    U = basis(&f5, NULL, 1, 0, NULL);
    snprintf(s, sizeof s, "projcg n=%" PRId64 " m=5 (fused)", n);
    projcg(s, &U, NULL, n, NULL, 6, 0);
    snprintf(s, sizeof s, "projcg n=%" PRId64 " m=5 (fused), stopped at its limit", n);
    projcg(s, &U, NULL, n, NULL, 2, 1);
    /* factored basis over a dense generator, also with c given */
    U = basis(&f5, NULL, 0, 1, NULL);
    snprintf(s, sizeof s, "projcg n=%" PRId64 " m=5 factored, dense generator", n);
    projcg(s, &U, NULL, n, NULL, 6, 0);
    snprintf(s, sizeof s, "projcg n=%" PRId64 " m=5 factored, dense generator, c given", n);
    projcg(s, &U, NULL, n, vec_hash(5, 9, 0.1, 0.0), 6, 0);
    /* stacked: materialised, factored over the dense generator */
    lfpsqp_mat* Jb = mat_hash(nb, 5, 1, 1.0);
    snprintf(s, sizeof s, "factorize n=%" PRId64 " m=5 weighted (bounds)", nb);
    factors fb = factorize(s, Jb, nb, 5, B.sx, 1);
    U = basis(&fb, &B, 1, 0, NULL);
    snprintf(s, sizeof s, "projcg N=%" PRId64 " m=5 stacked", nb);
    projcg(s, &U, &B, nb, NULL, 6, 0);
    U = basis(&fb, &B, 0, 1, NULL);
    snprintf(s, sizeof s, "projcg N=%" PRId64 " m=5 stacked, factored, dense generator", nb);
    projcg(s, &U, &B, nb, NULL, 6, 0);
    /* factored on a sparse twin with one dense extra column: plain and stacked (the tmpN region) */
    lfpsqp_spmat* SA = sparse_block(n, 4);
    lfpsqp_mat* As = dense_twin(SA, n, 4, 1);
    snprintf(s, sizeof s, "factorize n=%" PRId64 " m=4+1 (dense twin of a sparse block)", n);
    factors fs = factorize(s, As, n, 5, NULL, 0);
    U = basis(&fs, NULL, 0, 1, SA);
    snprintf(s, sizeof s, "projcg n=%" PRId64 " m=5 factored on the sparse twin + 1 dense column", n);
    projcg(s, &U, NULL, n, NULL, 6, 0);
    lfpsqp_spmat* SAb = sparse_block(nb, 4);
    lfpsqp_mat* Asb = dense_twin(SAb, nb, 4, 1);
    snprintf(s, sizeof s, "factorize n=%" PRId64 " m=4+1 weighted (dense twin, bounds)", nb);
    factors fsb = factorize(s, Asb, nb, 5, B.sx, 0);
    U = basis(&fsb, &B, 0, 1, SAb);
    snprintf(s, sizeof s, "projcg N=%" PRId64 " m=5 stacked, factored on the sparse twin + 1 dense column", nb);
    projcg(s, &U, &B, nb, NULL, 6, 0);
}

/* ---- lfpsqp_projcg_lowrank ---------------------------------------------------------------------------------------------------------- */
static void walk_lowrank(int64_t n) {
    char s[160];
    lfpsqp_mat* J = mat_hash(n, 5, 1, 1.0);
    factors f = factorize("factorize (low-rank solves)", J, n, 5, NULL, 1);
    const lfpsqp_basis U = basis(&f, NULL, 1, 0, NULL);
    for (int k = 1; k <= 8; k += 7) {
        const lfpsqp_lowrank_op A = {0.0, vec_hash(n, 3, 4.0, 5.0), mat_hash(n, k, 17, 0.25), k, NULL};
        lfpsqp_vec *x = vec(n), *lam = vec(6), *rhs = vec_hash(n, 4, 1.0, 0.0);
        lfpsqp_projcg_work w = work(n, 5);
        int64_t iters = -1;
        double nr = -1.0;
        snprintf(s, sizeof s, "projcg_lowrank n=%" PRId64 " m=5 k=%d", n, k);
        STEP(s, lfpsqp_projcg_lowrank(ctx, x, lam, &A, &U, rhs, NULL, 0.0, 6, n, LFPSQP_PROJCG_WANT_LAMBDA, &w, &iters, &nr));
    }
}

/* ---- the coupled operators ------------------------------------------------------------------------------------------------------------ */
enum { TRIDIAG, BAND, DIAGS, STENCIL, SPARSE };
static const char* coupled_name[] = {"projcg_tridiag", "projcg_band bw=4", "projcg_diags K=4", "projcg_stencil K=13", "projcg_sparse width 32"};
static lfpsqp_sphess* graph(int64_t n, double scale) { /* rows i and i + k, k = 1 .. 16: 32 neighbours in the interior */
    const int64_t cap = 16 * n;
    int64_t* rows = (int64_t*)host(sizeof(int64_t) * (size_t)cap);
    int64_t* cols = (int64_t*)host(sizeof(int64_t) * (size_t)cap);
    double* vals = hostd(cap);
    int64_t nnz = 0;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = 1; k <= 16 && i + k < n; ++k) {
            rows[nnz] = i; cols[nnz] = i + k; vals[nnz] = scale * unit((uint64_t)(16 * i + k));
            ++nnz;
        }
    lfpsqp_sphess* S = NULL;
    CK(lfpsqp_sphess_create(ctx, n, nnz, rows, cols, vals, &S));
    return shpool[nsh_++] = S;
}
static void coupled(int kind, const char* form, const lfpsqp_basis* U, const bounds* b, int64_t n, double scale) {
    static const int64_t d4[4] = {1, 7, 8, 9};
    static const int64_t d13[13] = {1, 2, 3, 5, 6, 7, 30, 31, 32, 35, 36, 37, 41};
    const int64_t nv = b ? b->nv : n, m = U->ncols, ng = b ? 2 * n : n;
    lfpsqp_vec* dg = b ? stacked_hash(n, 3, 4.0, 5.0) : vec_hash(n, 3, 4.0, 5.0);
    lfpsqp_vec* rhs = b ? stacked_hash(n, 4, 1.0, 0.0) : vec_hash(n, 4, 1.0, 0.0);
    lfpsqp_vec *x = vec(nv), *lam = vec((b ? n : 0) + m + 1), *Av = vec(nv);
    lfpsqp_projcg_work w = work(nv, m);
    int64_t iters = -1;
    double nr = -1.0;
    char s[200];
    snprintf(s, sizeof s, "%s n=%" PRId64 " m=%" PRId64 " %s", coupled_name[kind], n, m, form);
    const int fl = LFPSQP_PROJCG_WANT_LAMBDA;
    if (kind == TRIDIAG) {
        const lfpsqp_tridiag_op A = {0.0, dg, vec_hash(n, 15, scale, 0.0)};
        STEP(s, lfpsqp_projcg_tridiag(ctx, x, lam, &A, Av, U, rhs, NULL, 0.0, 6, ng, fl, &w, &iters, &nr));
    } else if (kind == BAND) {
        STEP(s, lfpsqp_projcg_band(ctx, x, lam, 0.0, dg, mat_hash(n, 4, 15, scale), 4, Av, U, rhs, NULL, 0.0, 6, ng, fl, &w, &iters, &nr));
    } else if (kind == DIAGS) {
        STEP(s, lfpsqp_projcg_diags(ctx, x, lam, 0.0, dg, mat_hash(n, 4, 15, scale), 4, d4, Av, U, rhs, NULL, 0.0, 6, ng, fl, &w, &iters, &nr));
    } else if (kind == STENCIL) {
        STEP(s, lfpsqp_projcg_stencil(ctx, x, lam, 0.0, dg, mat_hash(n, 13, 15, scale), 13, d13, Av, U, rhs, NULL, 0.0, 6, ng, fl, &w, &iters, &nr));
    } else {
        STEP(s, lfpsqp_projcg_sparse(ctx, x, lam, 0.0, dg, graph(n, scale), Av, U, rhs, NULL, 0.0, 6, ng, fl, &w, &iters, &nr));
    }
}
static void walk_coupled(int64_t n, int64_t nb) {
    const bounds B = make_bounds(nb);
    lfpsqp_mat* J = mat_hash(n, 5, 1, 1.0);
    factors f = factorize("factorize (coupled solves)", J, n, 5, NULL, 1);
    lfpsqp_mat* Jb = mat_hash(nb, 5, 1, 1.0);
    factors fb = factorize("factorize weighted (coupled solves, bounds)", Jb, nb, 5, B.sx, 1);
    const lfpsqp_basis U = basis(&f, NULL, 1, 0, NULL), Uf = basis(&f, NULL, 0, 1, NULL), Ub = basis(&fb, &B, 1, 0, NULL);
    for (int kind = TRIDIAG; kind <= SPARSE; ++kind) {
        coupled(kind, "plain", &U, NULL, n, 0.05);
        coupled(kind, "stacked", &Ub, &B, nb, 0.05);
    }
    coupled(DIAGS, "plain, factored basis", &Uf, NULL, n, 0.05);
    /* couplings that are not diagonally dominant: the negative-weight Gram pass runs */
    coupled(BAND, "plain, not diagonally dominant", &U, NULL, n, 8.0);
    coupled(SPARSE, "stacked, not diagonally dominant", &Ub, &B, nb, 8.0);
}

/* ---- lfpsqp_tangent_step, then lfpsqp_projcg from the state it leaves ------------------------------------------------------------------- */
static void walk_tangent(int64_t n, int init) {
    const int64_t m = 5;
    char s[160];
    lfpsqp_mat* J = mat_hash(n, m, 1, 1.0);
    lfpsqp_vec* d = vec_hash(n, 21, 1.0, 0.0);
    double *Sigma = hostd(m), *Vt = hostd(m * m), *W = hostd(m * m), *Jtd = hostd(m), *G = hostd(m * m), *Utd = hostd(m), *lam = hostd(m);
    int64_t rank = 0;
    snprintf(s, sizeof s, "factorize_rhs n=%" PRId64 " m=5 (factors only)", n);
    STEP(s, lfpsqp_factorize_rhs(ctx, J, NULL, NULL, Sigma, Vt, W, &rank, 1e-10, d, Jtd, G));
    lfpsqp_basis U;
    memset(&U, 0, sizeof U);
    U.ncols = rank; U.A = J; U.W = W;
    lfpsqp_vec* hdiag = vec_hash(n, 3, 4.0, 5.0);
    lfpsqp_projcg_work w = work(n, m);
    double dss = 0.0;
    snprintf(s, sizeof s, "tangent_step n=%" PRId64 " m=5%s", n, init ? " with the folded initial projection" : "");
    STEP(s, lfpsqp_tangent_step(ctx, &U, Sigma, Vt, m, Jtd, G, d, NULL, NULL, hdiag, NULL, NULL, NULL, NULL, &w, init ? LFPSQP_TANGENT_INIT_PROJCG : 0,
                                Utd, lam, &dss));
    const lfpsqp_diag_op A = {0.0, hdiag};
    lfpsqp_vec* x = vec(n);
    int64_t iters = -1;
    double nr = -1.0;
    snprintf(s, sizeof s, "  ... projcg %s", init ? "START_PROJECTED" : "START_GIVEN");
    STEP(s, lfpsqp_projcg(ctx, x, NULL, &A, &U, d, NULL, 0.0, 6, n, init ? LFPSQP_PROJCG_START_PROJECTED : LFPSQP_PROJCG_START_GIVEN, &w, &iters, &nr));
}

/* ---- lfpsqp_retract_nr -------------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int64_t n, m;
    double* J; /* host copy, n x m */
    double* x; /* host scratch, n */
} host_cons;
static int host_c(void* user, const lfpsqp_vec* x, double* cval) { /* c(x) = J'x on the host */
    host_cons* h = (host_cons*)user;
    if (lfpsqp_vec_download(ctx, x, 0, h->x, h->n) != 0) return 1;
    for (int64_t j = 0; j < h->m; ++j) {
        double a = 0.0;
        for (int64_t i = 0; i < h->n; ++i) a += h->J[j * h->n + i] * h->x[i];
        cval[j] = a;
    }
    return 0;
}
static void retract_nr(const char* what, const factors* f, const lfpsqp_basis* U, const bounds* b, const lfpsqp_spmat* Jsp, int use_cfun) {
    const int64_t n = f->n, m = f->m, nv = b ? b->nv : n;
    lfpsqp_constraints cons;
    memset(&cons, 0, sizeof cons);
    cons.Jct = f->J; cons.m_lin = m; cons.b = hostd(m); cons.n_x = n; cons.slack_row = -1; cons.Jsp = Jsp;
    lfpsqp_vec* x = b ? b->xaug : vec(n);
    lfpsqp_vec *xtilde = vec(nv), *xnew = vec(nv);
    CK(lfpsqp_vec_copy(ctx, xtilde, x));
    CK(lfpsqp_vec_copy_range(ctx, xtilde, 0, vec_hash(n, 41, 0.01, 0.0), 0, n));
    if (b) CK(lfpsqp_axpby(ctx, 1.0, x, 1.0, xtilde));
    host_cons hc = {n, m, NULL, NULL};
    if (use_cfun) {
        hc.J = hostd(n * m); hc.x = hostd(n);
        CK(lfpsqp_mat_download(ctx, f->J, 0, m, hc.J, n));
    }
    double* cval = hostd(m);
    int flag = -1;
    int64_t iters = -1;
    STEP(what, lfpsqp_retract_nr(ctx, U, f->Sigma, f->Vt, m, use_cfun ? NULL : &cons, use_cfun ? host_c : NULL, &hc, b ? &b->id : NULL, xtilde, x, xnew,
                                 1e-9, 6, cval, &flag, &iters));
}
static void walk_retract_nr(int64_t n, int64_t nb) {
    char s[160];
    const bounds B = make_bounds(nb);
    lfpsqp_mat* J = mat_hash(n, 5, 1, 1.0);
    factors f = factorize("factorize (Newton retractions)", J, n, 5, NULL, 1);
    lfpsqp_basis U = basis(&f, NULL, 1, 0, NULL);
    snprintf(s, sizeof s, "retract_nr n=%" PRId64 " m=5 device loop", n);
    retract_nr(s, &f, &U, NULL, NULL, 0);
    snprintf(s, sizeof s, "retract_nr n=%" PRId64 " m=5 host loop (cfun callback)", n);
    retract_nr(s, &f, &U, NULL, NULL, 1);
    U = basis(&f, NULL, 1, 1, NULL);
    snprintf(s, sizeof s, "retract_nr n=%" PRId64 " m=5 device loop, generator known", n);
    retract_nr(s, &f, &U, NULL, NULL, 0);
    lfpsqp_mat* Jb = mat_hash(nb, 5, 1, 1.0);
    factors fb = factorize("factorize weighted (Newton retractions, bounds)", Jb, nb, 5, B.sx, 1);
    U = basis(&fb, &B, 1, 0, NULL);
    snprintf(s, sizeof s, "retract_nr N=%" PRId64 " m=5 device loop with bounds", nb);
    retract_nr(s, &fb, &U, &B, NULL, 0);
    U = basis(&fb, &B, 1, 1, NULL);
    snprintf(s, sizeof s, "retract_nr N=%" PRId64 " m=5 device loop with bounds, generator known", nb);
    retract_nr(s, &fb, &U, &B, NULL, 0);
    lfpsqp_spmat* Jsp = sparse_block(n, 5);
    lfpsqp_mat* Js = dense_twin(Jsp, n, 5, 0);
    factors fs = factorize("factorize (dense twin of a sparse block)", Js, n, 5, NULL, 1);
    U = basis(&fs, NULL, 1, 1, NULL);
    snprintf(s, sizeof s, "retract_nr n=%" PRId64 " m=5 device loop, sparse twin", n);
    retract_nr(s, &fs, &U, NULL, Jsp, 0);
}

/* ---- lfpsqp_retract_nr_batch ----------------------------------------------------------------------------------------------------------- */
static void retract_batch(int64_t n, int64_t m, int nb, int mode) {
    char s[160];
    lfpsqp_mat* J = mat_hash(n, m, 1, 1.0);
    snprintf(s, sizeof s, "factorize n=%" PRId64 " m=%" PRId64 " (batched retraction)", n, m);
    factors f = factorize(s, J, n, m, NULL, 1);
    const lfpsqp_basis U = basis(&f, NULL, 1, 1, NULL);
    lfpsqp_constraints cons;
    memset(&cons, 0, sizeof cons);
    cons.Jct = J; cons.m_lin = m; cons.b = hostd(m); cons.n_x = n; cons.slack_row = -1;
    CK(lfpsqp_ctx_set_nr_batch_mode(ctx, mode));
    lfpsqp_vec* x = vec(n);
    const lfpsqp_vec* xtilde[16];
    lfpsqp_vec* xnew[16];
    for (int b = 0; b < nb; ++b) {
        xtilde[b] = vec_hash(n, 50 + (uint64_t)b, 0.01, 0.0);
        xnew[b] = vec(n);
    }
    double* cval = hostd(nb * m);
    int flags[16];
    int64_t iters[16];
    snprintf(s, sizeof s, "retract_nr_batch n=%" PRId64 " m=%" PRId64 " nb=%d %s", n, m, nb, mode == LFPSQP_NR_BATCH_EXACT ? "exact" : "matrix cores");
    STEP(s, lfpsqp_retract_nr_batch(ctx, &U, f.Sigma, f.Vt, m, &cons, NULL, nb, xtilde, x, xnew, 1e-9, 6, cval, flags, iters));
    CK(lfpsqp_ctx_set_nr_batch_mode(ctx, LFPSQP_NR_BATCH_EXACT));
}

/* ---- lfpsqp_pcg, lfpsqp_pcg_pre, lfpsqp_retract_pp ------------------------------------------------------------------------------------- */
static void walk_pcg(int64_t n, const bounds* b) {
    const int64_t m = 5, nv = b ? b->nv : n;
    char s[160];
    lfpsqp_basis Jop;
    memset(&Jop, 0, sizeof Jop);
    Jop.Z = mat_hash(n, m, 1, 1.0);
    Jop.ncols = m;
    if (b) { Jop.Dx = b->Dx; Jop.Dy = b->Dy; Jop.sx = vec_fill(n, 1.0); Jop.sy = vec(n); }
    int flag = -1;
    int64_t iters = -1;
    lfpsqp_vec* r = b ? stacked_hash(n, 4, 1.0, 0.0) : vec_hash(n, 4, 1.0, 0.0);
    snprintf(s, sizeof s, "pcg n=%" PRId64 " m=5 %s", n, b ? "stacked" : "plain");
    STEP(s, lfpsqp_pcg(ctx, 0.5, &Jop, vec(nv), r, vec(nv), vec(nv), b ? vec(n) : NULL, vec(m), 1e-10, 5, &flag, &iters));
    double* K = hostd(m * m);
    for (int64_t j = 0; j < m; ++j) K[j * m + j] = 0.5;
    lfpsqp_pcg_precond P;
    memset(&P, 0, sizeof P);
    P.K = K; P.q = vec(nv);
    if (b) { P.i11 = vec_fill(n, 2.0); P.i12 = vec(n); P.i22 = vec_fill(n, 2.0); }
    r = b ? stacked_hash(n, 4, 1.0, 0.0) : vec_hash(n, 4, 1.0, 0.0);
    snprintf(s, sizeof s, "pcg_pre n=%" PRId64 " m=5 %s", n, b ? "stacked" : "plain");
    STEP(s, lfpsqp_pcg_pre(ctx, 0.5, &Jop, &P, vec(nv), r, vec(nv), vec(nv), 1e-10, 5, &flag, &iters));
}
static void walk_retract_pp(int64_t n) {
    const int64_t m = 5;
    char s[160];
    lfpsqp_mat* J = mat_hash(n, m, 1, 1.0);
    lfpsqp_constraints cons;
    memset(&cons, 0, sizeof cons);
    cons.Jct = J; cons.m_lin = m; cons.b = hostd(m); cons.n_x = n; cons.slack_row = -1;
    lfpsqp_pp_work w;
    memset(&w, 0, sizeof w);
    w.r = vec(n); w.p = vec(n); w.z = vec(n); w.dx = vec(n); w.g = vec(n); w.tmp_m = vec(m);
    lfpsqp_vec *x = vec(n), *xtilde = vec_hash(n, 41, 0.1, 0.0), *xnew = vec(n);
    double* cval = hostd(m);
    int flag = -1;
    int64_t iters = -1, pcg_iters = -1;
    snprintf(s, sizeof s, "retract_pp n=%" PRId64 " m=5, two Gauss-Newton steps", n);
    STEP(s, lfpsqp_retract_pp(ctx, &cons, NULL, NULL, NULL, J, m, NULL, NULL, NULL, NULL, xtilde, x, xnew, 1.0, 1e-14, 2, 50, &w, cval, &flag, &iters,
                              &pcg_iters));
}

/* ---- the basis-forming product ----------------------------------------------------------------------------------------------------------- */
static void walk_rmul(int64_t n, int64_t k) {
    char s[160];
    lfpsqp_mat *In = mat_hash(n, k, 1, 1.0), *Out = mat(n, k);
    double* W = hostd(k * k);
    for (int64_t i = 0; i < k * k; ++i) W[i] = unit((uint64_t)i);
    snprintf(s, sizeof s, "rmul n=%" PRId64 " kcols=%" PRId64, n, k);
    STEP(s, lfpsqp_rmul(ctx, In, k, W, k, Out));
}

int main(void) {
    CK(lfpsqp_ctx_create(0, &ctx));
    static const int64_t ns[2] = {77, 2049};
    for (int k = 0; k < 2; ++k) {
        const int64_t n = ns[k];
        walk_projcg(n, 301);
        walk_lowrank(n);
        walk_coupled(n, 301);
        walk_tangent(n, 0);
        walk_tangent(n, 1);
        walk_retract_nr(n, 301);
        retract_batch(n, 5, 2, LFPSQP_NR_BATCH_EXACT);
        retract_batch(n, 5, 3, LFPSQP_NR_BATCH_EXACT);
        retract_batch(n, 5, 16, LFPSQP_NR_BATCH_MATRIX_CORES);
        walk_pcg(n, NULL);
        walk_retract_pp(n);
        walk_rmul(n, 5);
    }
    retract_batch(2049, 133, 8, LFPSQP_NR_BATCH_MATRIX_CORES);
    walk_rmul(2049, 133);
    {
        const bounds B = make_bounds(301);
        walk_pcg(301, &B);
    }

    CK(lfpsqp_ctx_sync(ctx));
    for (int i = 0; i < nsh_; ++i) CK(lfpsqp_sphess_free(ctx, shpool[i]));
    for (int i = 0; i < nsp_; ++i) CK(lfpsqp_spmat_free(ctx, sppool[i]));
    for (int i = 0; i < nv_; ++i) CK(lfpsqp_vec_free(ctx, vpool[i]));
    for (int i = 0; i < nm_; ++i) CK(lfpsqp_mat_free(ctx, mpool[i]));
    CK(lfpsqp_ctx_destroy(ctx));
    for (int i = 0; i < nh_; ++i) free(hpool[i]);
    printf("%s\n", failed ? "layout walk: ERRORS" : "layout walk: every call returned 0");
    return failed;
}
