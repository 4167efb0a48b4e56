// hmpc_certify.h -- the certificate of one QP record (KKT point / Farkas ray), item by item.
//
// Everything hmpc_certify_batch computes per record, as plain inline functions that compile for the device (hipcc) and for
// the host (g++): what one stationarity entry is, one multiplier's share, one dynamics entry, one slack, one objective
// term, how the partial results of a record combine into the ten residuals of include/hmpc.h and how a class is judged.
// The kernel (hmpc_certify.hip) supplies the lane loop and the wave reductions; tests/host/certify_driver.cpp walks the same
// functions with one "lane" under AddressSanitizer.
//
// The definitions are those of tests/certificates.py residuals(), which evaluates the reference's three checkers
// (warm_start_hmpc/test/cart_pole_with_wall.py:171-268, restated for any controller in tests/kkt_checks.py) on the rows as
// written out (layout: include/hmpc.h), with the problem's UNSCALED matrices, in float64.
//
// A record is a flat list of items, in five groups; a lane takes every `step`-th item of each group:
//   dual row       n_dual entries        |lam|, |mu|, |rho|, |sigma| maxima; signs of mu, nu_lb, nu_ub; terms of the dual objective
//   stationarity   n_primal entries      gradient of the Lagrangian in x_t[j] / u_t[j]: a column of [Q; -A; F] or [R; -B; G]
//   dynamics       (T + 1) nx entries    x0 - x_0,  A x_t + B u_t - x_{t+1}                                    (status 0)
//   slacks         n_mu + 2 T nub rows   h - F x_t - G u_t,  ub - lo,  hi - ub  with (lo, hi) from `fix`        (status 0)
//   objective      T (nq + nr) + nqT     (Q x_t)_r^2, (R u_t)_r^2, (Q_T x_T)_r^2                               (status 0)
//   primal count   n_primal entries      entries of the primal row that are not NaN                             (status 1)
// NaN: every maximum here PROPAGATES a NaN (cert_max; fmax would drop it), every sum does by itself -- a NaN anywhere in a
// decided record's rows ends as a NaN residual, which fails.  The primal row of an infeasible record is all NaN by contract:
// it is counted, and read by nothing else.
#ifndef HMPC_CERTIFY_H
#define HMPC_CERTIFY_H

#include <math.h>
#include <stdint.h>

#include "hmpc.h"

#ifndef HMPC_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define HMPC_HD __host__ __device__ __forceinline__
#else
#define HMPC_HD inline
#endif
#endif

#define HMPC_CERT_CLASS_POLISHED 0
#define HMPC_CERT_CLASS_UNPOLISHED 1
#define HMPC_CERT_CLASS_INFEASIBLE 2
#define HMPC_CERT_CLASS_WEAK 3
#define HMPC_CERT_CLASS_SKIPPED 4

// The problem as the caller of hmpc_create stated it (hmpc_problem: row-major, unscaled) and the offsets of the two rows.
struct CertProb {
    int nx, nu, nub, nuc, T, nc, ncL, nq, nr, nqT, n_primal, n_dual;
    int o_mu, o_lb, o_ub, o_rho, o_sig; // dual row: lam | mu | nu_lb | nu_ub | rho | sigma
    int o_u;                            // primal row: x_0 .. x_T | u_0 .. u_{T-1}
    const double *A, *B, *F, *G, *h, *FL, *GL, *hL, *Q, *R, *QT; // (FL, GL, hL: the last stage, ncL rows)
};

HMPC_HD void cert_set_sizes(CertProb &p, int nx, int nu, int nub, int T, int nc, int ncL, int nq, int nr, int nqT)
{
    p.nx = nx; p.nu = nu; p.nub = nub; p.nuc = nu - nub; p.T = T; p.nc = nc; p.ncL = ncL; p.nq = nq; p.nr = nr; p.nqT = nqT;
    p.n_primal = (T + 1) * nx + T * nu;
    p.o_mu = (T + 1) * nx;
    p.o_lb = p.o_mu + (T - 1) * nc + ncL;
    p.o_ub = p.o_lb + T * nub;
    p.o_rho = p.o_ub + T * nub;
    p.o_sig = p.o_rho + T * nq + nqT;
    p.n_dual = p.o_sig + T * nr;
    p.o_u = (T + 1) * nx;
}

// doubles of the eleven matrices, in the order of hmpc_problem (one block: hmpc_create uploads it, the kernel stages it)
HMPC_HD size_t cert_matrix_doubles(const CertProb &p)
{
    return (size_t)p.nx * p.nx + (size_t)p.nx * p.nu + (size_t)p.nc * (p.nx + p.nu + 1) + (size_t)p.ncL * (p.nx + p.nu + 1) +
           (size_t)p.nq * p.nx + (size_t)p.nr * p.nu + (size_t)p.nqT * p.nx;
}

HMPC_HD void cert_set_matrices(CertProb &p, const double *m)
{
    p.A = m; m += (size_t)p.nx * p.nx;
    p.B = m; m += (size_t)p.nx * p.nu;
    p.F = m; m += (size_t)p.nc * p.nx;
    p.G = m; m += (size_t)p.nc * p.nu;
    p.h = m; m += p.nc;
    p.FL = m; m += (size_t)p.ncL * p.nx;
    p.GL = m; m += (size_t)p.ncL * p.nu;
    p.hL = m; m += p.ncL;
    p.Q = m; m += (size_t)p.nq * p.nx;
    p.R = m; m += (size_t)p.nr * p.nu;
    p.QT = m;
}

// Compensated sum (Ogita, Rump, Oishi: Sum2 / Dot2): the rounding error of every addition (TwoSum) and of every product (one
// fused multiply-add) is kept in `c`, so the value is the sum as if accumulated in twice the precision and rounded once --
// WHATEVER the order of the terms.  The residuals are what is left when terms of size |h|, |F x|, |mu| cancel to ~1e-12: in
// plain float64 a serial loop, 64 lanes with a butterfly and numpy's order differ there by more than the reference's own
// rounding noise (measured on configs[4]: 7.9e-15 against 1.7e-15 in the primal inequality); compensated, all of them agree
// with the extended-precision reference to the last bit or two.  The sequences below must not be contracted or reassociated.
// clang (hipcc: the library is built with -ffp-contract=fast) takes the pragma inside each function; g++ takes the attribute.
// Any other host compiler must build this header without contraction and without -ffast-math; tests/host/certify_driver.cpp
// refuses to run where the sequences do not hold (cert_sum_self_test).
#if defined(__GNUC__) && !defined(__clang__)
#define HMPC_CERT_EXACT __attribute__((optimize("fp-contract=off", "no-fast-math")))
#else
#define HMPC_CERT_EXACT
#endif
struct CertSum { double s, c; };

HMPC_CERT_EXACT HMPC_HD void cert_sum_add(CertSum &a, double v)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double t = a.s + v, z = t - a.s;
    a.c += (a.s - (t - z)) + (v - z);
    a.s = t;
}

HMPC_CERT_EXACT HMPC_HD void cert_sum_mul(CertSum &a, double x, double y) // += x y
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double q = x * y, e = fma(x, y, -q);
    cert_sum_add(a, q);
    a.c += e;
}

// two partial sums into one (symmetric in its arguments: both lanes of a butterfly step end with the same bits)
HMPC_CERT_EXACT HMPC_HD void cert_sum_merge(CertSum &a, const CertSum &b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double t = a.s + b.s, z = t - a.s;
    const double e = (a.s - (t - z)) + (b.s - z); // exactly (a.s + b.s) - t, whichever comes first
    a.c = (a.c + b.c) + e;
    a.s = t;
}

HMPC_HD double cert_sum_value(const CertSum &a)
{
    const double r = a.s + a.c;
    return (r != r && a.s == a.s) ? a.s : r; // (an infinite sum stays infinite: its compensation is NaN)
}

// The three sequences on inputs whose rounding errors are known: 1 + 2^-60 - 1 and (1 + 2^-30)^2 - 1 - 2^-29 are both exactly
// 2^-60, which plain, contracted or reassociated float64 arithmetic does not return.
inline bool cert_sum_self_test()
{
    volatile double one = 1.0, tiny = ldexp(1.0, -60), x = 1.0 + ldexp(1.0, -30), step = ldexp(1.0, -29);
    CertSum a = {0.0, 0.0}, b = {0.0, 0.0}, c = {one, 0.0}, d = {-one, tiny};
    cert_sum_add(a, one); cert_sum_add(a, tiny); cert_sum_add(a, -one);
    cert_sum_mul(b, x, x); cert_sum_add(b, -one); cert_sum_add(b, -step);
    cert_sum_merge(c, d);
    return cert_sum_value(a) == tiny && cert_sum_value(b) == tiny && cert_sum_value(c) == tiny;
}

// What the items of a record add up to: a lane's share, then (after the reductions) the record's.
struct CertAcc {
    double max_lam, max_mu, max_rho, max_sig; // |.|_inf of the four segments
    double stat, neg;                         // max |stationarity entry|; max(0, -multiplier) over mu, nu_lb, nu_ub
    double peq, pineq;                        // max |dynamics entry|; max(0, -slack)
    CertSum dobj, pobj;                       // sums: dual objective, primal objective
    double count;                             // non-NaN primal entries (a small integer: exact)
};

HMPC_HD void cert_clear(CertAcc &a)
{
    a.max_lam = a.max_mu = a.max_rho = a.max_sig = a.stat = a.neg = a.peq = a.pineq = 0.0;
    a.dobj.s = a.dobj.c = a.pobj.s = a.pobj.c = a.count = 0.0;
}

// max that keeps a NaN once it has seen one (fmax(NaN, x) = x would lose it)
HMPC_HD double cert_max(double m, double v) { return (v > m || v != v) ? v : m; }

// Python's max(a, b) of two floats, which is what combines two segments in tests/certificates.py: b if b > a else a -- a NaN in
// the SECOND argument is dropped there, and here, so that NaN lands in the same columns as on the host (every such NaN still
// reaches another residual of its record's list through the sums: it fails either way)
HMPC_HD double cert_max_of_two(double a, double b) { return b > a ? b : a; }

HMPC_HD void cert_merge(CertAcc &a, const CertAcc &b)
{
    a.max_lam = cert_max(a.max_lam, b.max_lam); a.max_mu = cert_max(a.max_mu, b.max_mu);
    a.max_rho = cert_max(a.max_rho, b.max_rho); a.max_sig = cert_max(a.max_sig, b.max_sig);
    a.stat = cert_max(a.stat, b.stat); a.neg = cert_max(a.neg, b.neg);
    a.peq = cert_max(a.peq, b.peq); a.pineq = cert_max(a.pineq, b.pineq);
    cert_sum_merge(a.dobj, b.dobj); cert_sum_merge(a.pobj, b.pobj); a.count += b.count;
}

// bounds of binary (t, i) under the identifier: (0, 1) free, (v, v) fixed (controller.py:273-298)
HMPC_HD double cert_lo(const int8_t *fix, int k) { return fix[k] >= 0 ? (double)fix[k] : 0.0; }
HMPC_HD double cert_hi(const int8_t *fix, int k) { return fix[k] >= 0 ? (double)fix[k] : 1.0; }

// ---- dual row: entry i of d -------------------------------------------------------------------------------------------
// dual objective (kkt_checks.dual_objective):
//   - (|rho|^2 + |sigma|^2) / 4 - lam_0 . x0 + sum_t lo_t . nu_lb_t - hi_t . nu_ub_t - h . mu_t  (h_Tm1 for the last stage)
HMPC_HD void cert_dual_item(const CertProb &p, int i, const double *d, const double *x0, const int8_t *fix, CertAcc &a)
{
    const double v = d[i];
    if (i < p.o_mu) {
        a.max_lam = cert_max(a.max_lam, fabs(v));
        if (i < p.nx) cert_sum_mul(a.dobj, -v, x0[i]);
    } else if (i < p.o_lb) {
        const int k = i - p.o_mu, last = (p.T - 1) * p.nc;
        a.max_mu = cert_max(a.max_mu, fabs(v));
        a.neg = cert_max(a.neg, -v);
        cert_sum_mul(a.dobj, -(k < last ? p.h[k % p.nc] : p.hL[k - last]), v);
    } else if (i < p.o_ub) {
        a.neg = cert_max(a.neg, -v);
        cert_sum_mul(a.dobj, cert_lo(fix, i - p.o_lb), v);
    } else if (i < p.o_rho) {
        a.neg = cert_max(a.neg, -v);
        cert_sum_mul(a.dobj, -cert_hi(fix, i - p.o_ub), v);
    } else if (i < p.o_sig) {
        a.max_rho = cert_max(a.max_rho, fabs(v));
        cert_sum_mul(a.dobj, -0.25 * v, v);
    } else {
        a.max_sig = cert_max(a.max_sig, fabs(v));
        cert_sum_mul(a.dobj, -0.25 * v, v);
    }
}

// ---- stationarity: entry k of the gradient of the Lagrangian, numbered like the primal row (kkt_checks.dual_residuals) ----
//   x_t[j], t < T :  Q' rho_t + lam_t - A' lam_{t+1} + F_t' mu_t
//   x_T[j]        :  Q_T' rho_T + lam_T
//   u_t[j]        :  R' sigma_t - B' lam_{t+1} + G_t' mu_t + (nu_ub_t - nu_lb_t)[j - nuc]   (the binaries are the last nub inputs)
HMPC_HD double cert_stationarity_item(const CertProb &p, int k, const double *d)
{
    const int nx = p.nx, nu = p.nu, T = p.T;
    CertSum s = {0.0, 0.0};
    if (k < p.o_u) {
        const int t = k / nx, j = k - t * nx;
        if (t == T) {
            const double *rho = d + p.o_rho + T * p.nq;
            for (int r = 0; r < p.nqT; r++) cert_sum_mul(s, p.QT[r * nx + j], rho[r]);
            cert_sum_add(s, d[T * nx + j]);
            return cert_sum_value(s);
        }
        const double *rho = d + p.o_rho + t * p.nq, *lam1 = d + (t + 1) * nx, *mu = d + p.o_mu + t * p.nc;
        const double *F = t < T - 1 ? p.F : p.FL;
        const int rows = t < T - 1 ? p.nc : p.ncL;
        for (int r = 0; r < p.nq; r++) cert_sum_mul(s, p.Q[r * nx + j], rho[r]);
        cert_sum_add(s, d[t * nx + j]);
        for (int i = 0; i < nx; i++) cert_sum_mul(s, -p.A[i * nx + j], lam1[i]);
        for (int r = 0; r < rows; r++) cert_sum_mul(s, F[r * nx + j], mu[r]);
        return cert_sum_value(s);
    }
    const int t = (k - p.o_u) / nu, j = (k - p.o_u) - t * nu;
    const double *sig = d + p.o_sig + t * p.nr, *lam1 = d + (t + 1) * nx, *mu = d + p.o_mu + t * p.nc;
    const double *G = t < T - 1 ? p.G : p.GL;
    const int rows = t < T - 1 ? p.nc : p.ncL;
    for (int r = 0; r < p.nr; r++) cert_sum_mul(s, p.R[r * nu + j], sig[r]);
    for (int i = 0; i < nx; i++) cert_sum_mul(s, -p.B[i * nu + j], lam1[i]);
    for (int r = 0; r < rows; r++) cert_sum_mul(s, G[r * nu + j], mu[r]);
    if (j >= p.nuc) {
        cert_sum_add(s, d[p.o_ub + t * p.nub + (j - p.nuc)]);
        cert_sum_add(s, -d[p.o_lb + t * p.nub + (j - p.nuc)]);
    }
    return cert_sum_value(s);
}

// ---- primal row w (kkt_checks.primal_residuals, primal_objective) ---------------------------------------------------------------
// dynamics entry k in [0, (T + 1) nx):  x0 - x_0,  A x_t + B u_t - x_{t+1}
HMPC_HD double cert_dynamics_item(const CertProb &p, int k, const double *w, const double *x0)
{
    const int nx = p.nx, nu = p.nu;
    if (k < nx) return x0[k] - w[k];
    const int t = k / nx - 1, j = k - (t + 1) * nx;
    const double *x = w + t * nx, *u = w + p.o_u + t * nu;
    CertSum s = {0.0, 0.0};
    for (int i = 0; i < nx; i++) cert_sum_mul(s, p.A[j * nx + i], x[i]);
    for (int i = 0; i < nu; i++) cert_sum_mul(s, p.B[j * nu + i], u[i]);
    cert_sum_add(s, -w[k]);
    return cert_sum_value(s);
}

// rows of the slack list: the n_mu rows of [F G | h] stage by stage, then T nub lower and T nub upper bounds of the binaries
HMPC_HD int cert_slack_items(const CertProb &p) { return (p.T - 1) * p.nc + p.ncL + 2 * p.T * p.nub; }

HMPC_HD double cert_slack_item(const CertProb &p, int k, const double *w, const int8_t *fix)
{
    const int nx = p.nx, nu = p.nu, n_mu = (p.T - 1) * p.nc + p.ncL, nb = p.T * p.nub;
    if (k < n_mu) {
        const int last = (p.T - 1) * p.nc, t = k < last ? k / p.nc : p.T - 1, r = k < last ? k - t * p.nc : k - last;
        const double *F = k < last ? p.F : p.FL, *G = k < last ? p.G : p.GL;
        const double *x = w + t * nx, *u = w + p.o_u + t * nu;
        CertSum s = {k < last ? p.h[r] : p.hL[r], 0.0};
        for (int i = 0; i < nx; i++) cert_sum_mul(s, -F[r * nx + i], x[i]);
        for (int i = 0; i < nu; i++) cert_sum_mul(s, -G[r * nu + i], u[i]);
        return cert_sum_value(s);
    }
    k -= n_mu;
    const int q = k < nb ? k : k - nb, t = q / p.nub, i = q - t * p.nub;
    const double ub = w[p.o_u + t * nu + p.nuc + i];
    return k < nb ? ub - cert_lo(fix, q) : cert_hi(fix, q) - ub;
}

// terms of the primal objective: |Q x_t|^2 (T nq), |R u_t|^2 (T nr), |Q_T x_T|^2 (nqT)
HMPC_HD int cert_objective_items(const CertProb &p) { return p.T * (p.nq + p.nr) + p.nqT; }

HMPC_HD double cert_objective_item(const CertProb &p, int k, const double *w) // (the row's product; the term is its square)
{
    const int nx = p.nx, nu = p.nu, T = p.T;
    CertSum s = {0.0, 0.0};
    if (k < T * p.nq) {
        const int t = k / p.nq, r = k - t * p.nq;
        for (int i = 0; i < nx; i++) cert_sum_mul(s, p.Q[r * nx + i], w[t * nx + i]);
    } else if (k < T * (p.nq + p.nr)) {
        k -= T * p.nq;
        const int t = k / p.nr, r = k - t * p.nr;
        for (int i = 0; i < nu; i++) cert_sum_mul(s, p.R[r * nu + i], w[p.o_u + t * nu + i]);
    } else {
        const int r = k - T * (p.nq + p.nr);
        for (int i = 0; i < nx; i++) cert_sum_mul(s, p.QT[r * nx + i], w[T * nx + i]);
    }
    return cert_sum_value(s);
}

// ---- a lane's share of one record: items first, first + step, ... of every group (host: first = 0, step = 1) ----------------------
HMPC_HD void cert_accumulate(const CertProb &p, int status, const double *w, const double *d, const double *x0, const int8_t *fix,
                             int first, int step, CertAcc &a)
{
    for (int i = first; i < p.n_dual; i += step) cert_dual_item(p, i, d, x0, fix, a);
    for (int k = first; k < p.n_primal; k += step) a.stat = cert_max(a.stat, fabs(cert_stationarity_item(p, k, d)));
    if (status == HMPC_INFEASIBLE) { // the primal row of a ray is all NaN by contract: counted, and read by nothing else
        for (int k = first; k < p.n_primal; k += step) a.count += w[k] == w[k] ? 1.0 : 0.0;
        return;
    }
    for (int k = first; k < (p.T + 1) * p.nx; k += step) a.peq = cert_max(a.peq, fabs(cert_dynamics_item(p, k, w, x0)));
    const int ns = cert_slack_items(p), no = cert_objective_items(p);
    for (int k = first; k < ns; k += step) a.pineq = cert_max(a.pineq, -cert_slack_item(p, k, w, fix));
    for (int k = first; k < no; k += step) {
        const double v = cert_objective_item(p, k, w);
        cert_sum_mul(a.pobj, v, v);
    }
}

// ---- class of a record and the ten residuals from its (reduced) sums and maxima ---------------------------------------------------
HMPC_HD int cert_class(int status, int iters)
{
    if (status == HMPC_OPTIMAL) return (iters & HMPC_ITERS_POLISHED) ? HMPC_CERT_CLASS_POLISHED : HMPC_CERT_CLASS_UNPOLISHED;
    if (status == HMPC_INFEASIBLE) return (iters & HMPC_ITERS_WEAK) ? HMPC_CERT_CLASS_WEAK : HMPC_CERT_CLASS_INFEASIBLE;
    return HMPC_CERT_CLASS_SKIPPED;
}

HMPC_HD void cert_skipped(double *res)
{
    for (int c = 0; c < HMPC_CERT_COUNT; c++) res[c] = NAN;
}

HMPC_HD void cert_residuals(const CertAcc &a, int status, double obj, double dual_obj, double *res)
{
    cert_skipped(res);
    const double dobj = cert_sum_value(a.dobj), pobj = cert_sum_value(a.pobj);
    const double scale = 1.0 + cert_max_of_two(a.max_lam, a.max_mu);
    res[HMPC_CERT_STATIONARITY] = a.stat / scale;
    res[HMPC_CERT_SIGN] = a.neg / scale;
    res[HMPC_CERT_DUAL_OBJ] = fabs(dobj - dual_obj) / (1.0 + fabs(dobj));
    if (status == HMPC_INFEASIBLE) {
        res[HMPC_CERT_RAY_QUADRATIC] = cert_max_of_two(a.max_rho, a.max_sig);
        res[HMPC_CERT_RAY_OBJECTIVE] = dobj > 0.0 ? 0.0 : INFINITY;
        res[HMPC_CERT_RAY_PRIMAL] = a.count + (obj == INFINITY ? 0.0 : 1.0);
        return;
    }
    res[HMPC_CERT_PRIMAL_EQUALITY] = a.peq;
    res[HMPC_CERT_PRIMAL_INEQUALITY] = a.pineq;
    res[HMPC_CERT_OBJ] = fabs(pobj - obj) / (1.0 + fabs(pobj));
    res[HMPC_CERT_GAP] = fabs(pobj - dobj) / (1.0 + fabs(pobj));
}

// columns a class is held to (tests/certificates.py _names): a WEAK ray is exempt from the stationarity bound, and from that only
HMPC_HD unsigned cert_columns(int cls)
{
    const unsigned dual = 1u << HMPC_CERT_STATIONARITY | 1u << HMPC_CERT_SIGN | 1u << HMPC_CERT_DUAL_OBJ;
    const unsigned optimal = dual | 1u << HMPC_CERT_PRIMAL_EQUALITY | 1u << HMPC_CERT_PRIMAL_INEQUALITY | 1u << HMPC_CERT_OBJ | 1u << HMPC_CERT_GAP;
    const unsigned ray = dual | 1u << HMPC_CERT_RAY_QUADRATIC | 1u << HMPC_CERT_RAY_OBJECTIVE | 1u << HMPC_CERT_RAY_PRIMAL;
    if (cls == HMPC_CERT_CLASS_POLISHED || cls == HMPC_CERT_CLASS_UNPOLISHED) return optimal;
    if (cls == HMPC_CERT_CLASS_INFEASIBLE) return ray;
    if (cls == HMPC_CERT_CLASS_WEAK) return ray & ~(1u << HMPC_CERT_STATIONARITY);
    return 0u;
}

// verdict word of include/hmpc.h: class | HMPC_CERT_FAILED | failing columns << 16.  "Fails" is "not <= bound": NaN fails.
HMPC_HD int32_t cert_verdict(int cls, const double *res, const hmpc_cert_tol &tol)
{
    const double bound = cls == HMPC_CERT_CLASS_POLISHED ? tol.polished : cls == HMPC_CERT_CLASS_UNPOLISHED ? tol.unpolished :
                         cls == HMPC_CERT_CLASS_INFEASIBLE ? tol.infeasible : tol.weak;
    const unsigned held = cert_columns(cls);
    unsigned failing = 0;
    for (int c = 0; c < HMPC_CERT_COUNT; c++)
        if ((held >> c & 1u) && !(res[c] <= (c >= HMPC_CERT_RAY_QUADRATIC ? 0.0 : bound))) failing |= 1u << c;
    return (int32_t)(cls | (failing ? HMPC_CERT_FAILED : 0) | failing << 16);
}

HMPC_HD hmpc_cert_tol cert_default_tol()
{
    hmpc_cert_tol t;
    t.polished = 1e-8; t.unpolished = 5e-6; t.infeasible = 1e-6; t.weak = 1e-6;
    return t;
}

// ---- one record, start to end, on one "lane": the CPU form ----------------------------------------------------------------------
inline void cert_record_serial(const CertProb &p, int status, int iters, double obj, double dual_obj, const double *w, const double *d,
                               const double *x0, const int8_t *fix, const hmpc_cert_tol &tol, double *res, int32_t *verdict)
{
    const int cls = cert_class(status, iters);
    if (cls == HMPC_CERT_CLASS_SKIPPED) {
        cert_skipped(res);
    } else {
        CertAcc a;
        cert_clear(a);
        cert_accumulate(p, status, w, d, x0, fix, 0, 1, a);
        cert_residuals(a, status, obj, dual_obj, res);
    }
    if (verdict) *verdict = cert_verdict(cls, res, tol);
}

#endif // HMPC_CERTIFY_H
