/*
 * hmpc.h -- C ABI of the MI355X batched QP-relaxation solver for hybrid MPC.
 *
 * This is the drop-in boundary for ONE hot path of TobiaMarcucci/warm-start-hybrid-mpc:
 * the QP relaxation solved at every branch-and-bound node.  In the reference that path is
 *
 *   warm_start_hmpc/controller.py:365-376   solver(identifier, cutoff, extra) closure
 *   warm_start_hmpc/controller.py:229-271   _solve_subproblem  (set bounds, set x0, optimize)
 *   warm_start_hmpc/controller.py:273-298   _set_bound_binaries
 *   warm_start_hmpc/bounded_qp.py:200-228   BoundedQP.optimize (+ Farkas proof if infeasible)
 *   warm_start_hmpc/subproblem_solution.py:18-168  extraction of the primal/dual record
 *
 * and it bottoms out in Gurobi's C library through gurobipy.  The entry points below are
 * what a binding for that path needs: build the node-independent QP once (the role of
 * controller.py:119-184 _build_mip), then solve any number of nodes -- each given by its
 * vector of binary fixings and an initial state -- in one call.  Plain pointers and sizes
 * only; all matrices row-major float64.
 *
 * The QP of one node (reference statement: controller.py:47-56, 119-184):
 *
 *   min  sum_{t<T} |Q x_t|^2 + |R u_t|^2  +  |Q_T x_T|^2
 *   s.t. x_0 = x0                                  (multiplier lam_0)
 *        x_{t+1} = A x_t + B u_t                   (lam_{t+1})
 *        F x_t + G u_t <= h            t < T-1     (mu_t >= 0)
 *        F_Tm1 x_t + G_Tm1 u_t <= h_Tm1  t = T-1   (mu_{T-1} >= 0)
 *        lb_t <= ub_t <= ubmax_t                   (nu_lb_t, nu_ub_t >= 0)
 *
 * with u_t = (uc_t, ub_t), ub_t the last nub entries, and (lb, ubmax) = (0, 1) for a free
 * binary, (v, v) for a binary fixed to v.  Sign conventions are the reference's
 * (bounded_qp.py:260-332): inequality multipliers are nonnegative; an infeasible node has
 * objective +inf, no primal, and multipliers that form a Farkas proof whose "dual
 * objective" -sum(rhs * multiplier) is positive.
 */
#ifndef HMPC_H
#define HMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-node status (hmpc_result.status) */
#define HMPC_OPTIMAL 0
#define HMPC_INFEASIBLE 1
#define HMPC_MAXITER 2   /* not converged: the caller must not use the record */
#define HMPC_NUMERICAL 3 /* numerical breakdown: idem */
#define HMPC_UNBOUNDED 4 /* hmpc_lp_solve_batch only: the cost grows without bound on the set */

#define HMPC_ITERS_POLISHED 0x10000 /* flag in hmpc_result.iters */
#define HMPC_ITERS_WEAK 0x20000     /* flag in hmpc_result.iters: HMPC_INFEASIBLE, but the ray is no proof to tolerance */
#define HMPC_ITERS_TERMINAL 0x80000 /* flag in hmpc_result.iters (launches with hmpc_warm, and large cold batches in the two-launch form): the terminal-set rows were needed */
#define HMPC_ITERS_HANDED 0x40000   /* flag in hmpc_result.iters: the active set handed down by the parent (hmpc_warm) verified */
#define HMPC_ITERS_UNCERTIFIED 0x100000 /* flag in hmpc_result.iters, with HMPC_ITERS_WEAK: the node was pruned on the collapse of tau ALONE
                                         * (tau <= 1e-12 kappa), no ray met even the loose bound of the weak exit -- the drivers count
                                         * such prunes and say so when one removed a node whose bound lay below the final incumbent */

/* return codes */
#define HMPC_OK 0
#define HMPC_EINVAL -1 /* bad argument (sizes, null pointers) */
#define HMPC_EDEVICE -2 /* HIP error; text in hmpc_last_error() */
#define HMPC_ETOOBIG -3 /* the per-node vectors exceed one CU's LDS even with lists and factor in global memory */

/* Node-independent problem data (replaces the Gurobi model built by controller.py:119-184).
 * nc  = rows of [F G];  ncT = rows of [F_Tm1 G_Tm1] (= nc + terminal facets, controller.py:85-87).
 * nq, nr, nqT = rows of Q, R, Q_T. */
typedef struct hmpc_problem {
    int32_t nx, nu, nub, T, nc, ncT, nq, nr, nqT;
    const double *A;     /* nx  x nx */
    const double *B;     /* nx  x nu */
    const double *F;     /* nc  x nx */
    const double *G;     /* nc  x nu */
    const double *h;     /* nc       */
    const double *F_Tm1; /* ncT x nx */
    const double *G_Tm1; /* ncT x nu */
    const double *h_Tm1; /* ncT      */
    const double *Q;     /* nq  x nx */
    const double *R;     /* nr  x nu */
    const double *Q_T;   /* nqT x nx */
} hmpc_problem;

/* Solver options (the role of the reference's gurobi_params, controller.py:778-796). */
typedef struct hmpc_options {
    double tol;            /* optimality: scaled residuals and relative gap (default 1e-8)   */
    double tol_inf;        /* infeasibility proof: |A'y| <= tol_inf * (-b'y) (default 1e-6) */
    int32_t max_iter;      /* interior-point iterations per solve (default 100)             */
    int32_t lazy_terminal; /* 1: try each node without the terminal-set rows first          */
    int32_t refine;        /* 1: one step of iterative refinement per Newton direction      */
    int32_t device;        /* HIP device ordinal, -1 = current                              */
    int32_t polish;        /* 1: active-set polish -- an optimal node returns the vertex     */
                           /*    solution of its active set (what Gurobi's simplex/crossover */
                           /*    returns, bounded_qp.py:208), exactly complementary          */
    int32_t reserved;      /* 0                                                             */
    double polish_tol;     /* the polish is tried once residuals and gap are below this     */
                           /*    (default 1e-4; it is accepted only if it verifies)          */
} hmpc_options;

/* Structure-of-arrays result of a batch of B nodes.  Any pointer may be NULL (not wanted).
 * primal row (n_primal doubles): x_0..x_T (nx each), then u_0..u_{T-1} (nu each; uc then ub).
 *   NaN for an infeasible node.
 * dual row (n_dual doubles), in this order (subproblem_solution.py:142-166):
 *   lam_0..lam_T (nx) | mu_0..mu_{T-2} (nc), mu_{T-1} (ncT) | nu_lb_0.. (nub) | nu_ub_0.. (nub)
 *   | rho_0..rho_{T-1} (nq), rho_T (nqT) | sigma_0..sigma_{T-1} (nr)
 *   with rho_t = 2 Q x_t, rho_T = 2 Q_T x_T, sigma_t = 2 R u_t, zeros for an infeasible node. */
typedef struct hmpc_result {
    double *obj;      /* B : primal objective, +inf if infeasible (bounded_qp.py:292-311)      */
    double *dual_obj; /* B : dual objective / Farkas objective   (bounded_qp.py:313-332)      */
    int32_t *status;  /* B                                                                    */
    int32_t *iters;   /* B : interior-point iterations spent on the node (low 16 bits);       */
                      /*     bit 16 (HMPC_ITERS_POLISHED): the record is the polished vertex    */
                      /*     solution (exactly complementary), not the interior-point iterate.  */
                      /*     An OPTIMAL record WITHOUT the bit is the iterate that met the      */
                      /*     stopping test (gap <= tol = 1e-8, or 100 tol = 1e-6 at the floor   */
                      /*     of the barrier parameter; ON THE SCALED COST, see below): optimal  */
                      /*     to that tolerance and carrying its own KKT                         */
                      /*     certificate, but reproducible across arithmetic orders only to     */
                      /*     ~1e-4 in the trajectory.  Every optimal node of the cart-pole      */
                      /*     systems polishes; 2 % of BASELINE configs[4]'s do not;              */
                      /*     bit 17 (HMPC_ITERS_WEAK): infeasible by about the accuracy of the  */
                      /*     arithmetic -- the embedding's tau collapsed, the node has no point */
                      /*     feasible to tolerance and is pruned, but its ray misses the proof  */
                      /*     tolerance (tol_inf): it must not be carried to the next MPC step   */
                      /*     (hmpc_fleet_* and the Python drivers reopen such a leaf at a shift) */
    double *primal;   /* B x n_primal                                                         */
    double *dual;     /* B x n_dual                                                           */
} hmpc_result;
/* What a record owes the options it was solved with (tests/test_solver_options.py).
 *   Units of the stopping test.  The solver works on the cost scaled by 1 / H, H the largest entry of the cost's Hessian
 *     2 (Q'Q (+) R'R), 2 Q_T'Q_T, and tests  |p - d| <= tol (1 + min(|p|, |d|))  THERE.  In the caller's units the relative gap
 *     |obj - dual_obj| / (1 + |obj|) of an unpolished OPTIMAL record is therefore at most  tol max(1, H)  where the iterate met
 *     tol, and at most  100 tol max(1, H)  where it left at the floor of the barrier parameter (mu < 1e-11, residuals and gap within
 *     100 tol: the iteration has nothing more to give).  That exit has been measured only without refinement (refine = 0: the
 *     dual residual then grows as mu falls and the iterate never meets tol; 2.5e-5 on the cart-pole with walls, H = 36.4) and
 *     with tol = 1e-10, which an unpolished record does not follow below about 1e-7 / H.  A POLISHED record is a verified vertex
 *     and does not depend on tol.
 *   max_iter caps every solve of a node: iters & 0xFFFF <= max_iter, or 2 max_iter where the terminal set is tried lazily
 *     (lazy_terminal = 1 and ncT > nc: up to two solves).  A capped solve is the uncapped one cut off.
 *   A record of status >= HMPC_MAXITER carries none of HMPC_ITERS_POLISHED, _WEAK, _UNCERTIFIED, _HANDED (each is raised on the
 *     exit that decides a node); its rows and objectives are the last iterate's and promise nothing.
 *   polish = 0: nothing is handed down either (hmpc_warm is ignored: the cold records bit for bit, but for HMPC_ITERS_TERMINAL).
 *   tol, tol_inf, max_iter, polish_tol <= 0 are the defaults; lazy_terminal, refine, polish are taken as they stand. */

/* Parent -> child hand-down (nullable everywhere).  The reference hands the parent node's simplex basis to the child
 * (controller.py:260-264, 426; subproblem_solution.py:37-43, with Gurobi's dual simplex); here the child receives the
 * parent's RECORD: node b tries the active set of row index[b] of (primal, dual) -- rows in the layout of hmpc_result,
 * e.g. the output arrays of an earlier call; index[b] < 0: nothing handed down -- before its first interior-point
 * iteration, multipliers and proximal centre from the parent.  A child whose optimum lies on the parent's active set
 * (the branch that fixes a binary where the relaxation had it) then costs one factorisation and a few solves instead
 * of ~11 iterations, and returns with HMPC_ITERS_HANDED set; where the set does not verify the node is solved from
 * the cold start exactly as without the hand-down.  Only records of OPTIMAL nodes flagged HMPC_ITERS_POLISHED may be
 * handed down (their multipliers are exactly complementary), and only to nodes with the same initial state.  States,
 * cost and the inputs the cost sees do not depend on the hand-down; where multipliers (dependent active rows) or
 * cost-free inputs are not unique a handed-down solve may return another optimal choice than a cold one.
 * Host-pointer form: host arrays of `rows` rows; device-pointer form: device arrays (`rows` unused), and the rows must
 * not be output rows of the same call. */
typedef struct hmpc_warm {
    const double *primal; /* rows x n_primal */
    const double *dual;   /* rows x n_dual   */
    const int32_t *index; /* B : row of node b's parent, or -1 */
    int32_t rows;
} hmpc_warm;

typedef struct hmpc_handle hmpc_handle;

/* Copies the problem to the device, precomputes scalings and sparse row/column lists.
 * options may be NULL (defaults).  The handle is bound to one device and is not thread-safe; it owns one set of
 * device workspaces: at most ONE launch per handle may be in flight (the device-pointer forms are asynchronous --
 * synchronise the stream, or use one handle per stream, before launching on the same handle again). */
int hmpc_create(const hmpc_problem *problem, const hmpc_options *options, hmpc_handle **out);
int hmpc_destroy(hmpc_handle *h);

/* Row lengths of hmpc_result.primal / .dual for this problem. */
int hmpc_record_sizes(const hmpc_handle *h, int32_t *n_primal, int32_t *n_dual);

/* Solves B nodes.  fix: B x (T*nub) int8, entry (t*nub+i) = -1 free, 0 or 1 fixed
 * (the identifier dictionaries of controller.py:273-298 flattened).  x0: nx doubles shared by
 * all nodes when x0_stride == 0, else B rows of stride x0_stride.
 * Host-pointer form: copies in, runs, copies out, returns when done.  Replaces
 * B calls of controller.py:229-271. */
int hmpc_solve_batch(hmpc_handle *h, const double *x0, int32_t x0_stride, const int8_t *fix, int32_t B,
                     const hmpc_warm *warm /* nullable */, const hmpc_result *out);

/* Device-pointer form: every pointer (x0, fix, and the members of out) is device memory on the
 * handle's device; the launch is asynchronous on `stream` (a hipStream_t, NULL = default stream). */
int hmpc_solve_batch_device(hmpc_handle *h, const double *d_x0, int32_t x0_stride, const int8_t *d_fix, int32_t B,
                            const hmpc_warm *d_warm /* nullable */, const hmpc_result *d_out, void *stream);

/* ---- Warm-start node shift (reference: controller.py:431-564 construct_warm_start, :615-721) --------
 * After an MPC step the leaves of the branch-and-bound tree become the initial cover of the next
 * step's tree: leaves that disagree with the applied binaries are dropped (controller.py:566-613),
 * identifiers and multipliers move one stage towards the present, the last stage is filled through
 * two precomputed maps (:635-666), and the dual objective -- the leaf's new lower bound -- changes
 * by the pi-sum of :668-721, then by the model error and the clipping / reopening rule of :541-558.
 * One wavefront per leaf; the kernel is memory bound (it reads and writes one dual row per leaf). */
typedef struct hmpc_shift_maps {
    const double *M_mu;  /* nc x ncT : mu'_{T-2}  = M_mu  mu_{T-1}   (controller.py:186-227 _update_mu) */
    const double *M_rho; /* nq x nqT : rho'_{T-1} = M_rho rho_T                                        */
    const double *V;     /* nub x nu : the binaries of an input vector (MLDSystem.V)                    */
} hmpc_shift_maps;
int hmpc_set_shift_maps(hmpc_handle *h, const hmpc_shift_maps *maps);

/* Shifts B leaves that belong to K trees (MPC instances advanced together).  owner[b] in [0, K) is the
 * tree of leaf b; x0, u0, e0 hold K rows: the state the step started from, the applied input (uc, ub)
 * and the model error of the step.  Per leaf in: fix (T*nub int8), lower bound (+inf: proved infeasible),
 * dual row, dual objective.  Per leaf out: shifted fix / dual row / dual objective, the new lower bound,
 * and flags: bit 0 = keep (the leaf agrees with the applied binaries; otherwise the other outputs are
 * undefined), bit 1 = reopened (its infeasibility proof did not survive the shift: lb = 0, multipliers
 * to be ignored).  Host-pointer form: copies in, runs, copies out. */
int hmpc_shift_batch(hmpc_handle *h, int32_t B, int32_t K, const int32_t *owner, const double *x0, const double *u0,
                     const double *e0, const int8_t *fix, const double *lb, const double *dual, const double *dual_obj,
                     int8_t *fix_out, double *lb_out, double *dual_out, double *dual_obj_out, uint8_t *flags);
/* Device-pointer form, asynchronous on `stream`. */
int hmpc_shift_batch_device(hmpc_handle *h, int32_t B, int32_t K, const int32_t *d_owner, const double *d_x0,
                            const double *d_u0, const double *d_e0, const int8_t *d_fix, const double *d_lb,
                            const double *d_dual, const double *d_dual_obj, int8_t *d_fix_out, double *d_lb_out,
                            double *d_dual_out, double *d_dual_obj_out, uint8_t *d_flags, void *stream);

/* ---- Certificates of a batch of records (KKT point / Farkas ray) ------------------------------------------
 * Every record of hmpc_result carries its own certificate: an OPTIMAL node is a KKT point, an INFEASIBLE node a Farkas
 * ray.  These entries evaluate it on the device, one wavefront per record (csrc/hmpc_certify.hip), from the rows AS
 * WRITTEN OUT and the problem's UNSCALED matrices, in float64 -- nothing the solver computed for itself is trusted, obj
 * and dual_obj included.  The conditions are the reference's three checkers (warm_start_hmpc/test/cart_pole_with_wall.py:
 * 171-268: primal feasibility, dual feasibility = stationarity + sign, dual objective), scaled as tests/kkt_checks.py
 * check_solution scales them; column by column the residuals are those of tests/certificates.py residuals():
 *   stationarity      max |gradient of the Lagrangian in x_t, u_t|          / (1 + max(|lam|_inf, |mu|_inf))
 *   sign              most negative of mu, nu_lb, nu_ub (0 if none)         / (1 + max(|lam|_inf, |mu|_inf))
 *   dual_obj          |dual objective of the multipliers - dual_obj| / (1 + |dual objective of the multipliers|)
 *   primal_equality   max |x_0 - x0|, |A x_t + B u_t - x_{t+1}|
 *   primal_inequality largest violation of [F G] rows, terminal rows and the bounds of the binaries under `fix`
 *   obj, gap          |cost of the primal row - obj|, |cost of the primal row - dual objective|, / (1 + |cost|)
 *   ray_quadratic     max |rho|, |sigma| beside a ray        (EXACT: must be 0)
 *   ray_objective     0 if the ray's dual objective is > 0, +inf otherwise (EXACT)
 *   ray_primal        non-NaN entries of the primal row, + 1 for an obj that is not +inf (EXACT)
 * A NaN anywhere in the rows of a decided record ends as a NaN residual, and NaN fails. */
/* columns of the residual matrix, in this order; NaN where a column does not apply to the record's status */
#define HMPC_CERT_STATIONARITY      0
#define HMPC_CERT_SIGN              1
#define HMPC_CERT_DUAL_OBJ          2
#define HMPC_CERT_PRIMAL_EQUALITY   3   /* status 0 only */
#define HMPC_CERT_PRIMAL_INEQUALITY 4   /* status 0 only */
#define HMPC_CERT_OBJ               5   /* status 0 only */
#define HMPC_CERT_GAP               6   /* status 0 only */
#define HMPC_CERT_RAY_QUADRATIC     7   /* status 1 only */
#define HMPC_CERT_RAY_OBJECTIVE     8   /* status 1 only: 0 or +inf */
#define HMPC_CERT_RAY_PRIMAL        9   /* status 1 only */
#define HMPC_CERT_COUNT            10

/* verdict[b]: low byte = class (0 polished: OPTIMAL with HMPC_ITERS_POLISHED -- a handed-down record is one --, 1 unpolished,
 * 2 infeasible, 3 weak: INFEASIBLE with HMPC_ITERS_WEAK, 4 skipped: status > 1, all residuals NaN, never failed);
 * HMPC_CERT_FAILED set when a residual of the class's list exceeds its tolerance or is NaN (the EXACT columns: is not 0; a weak
 * ray is exempt from the stationarity bound, and from that only);
 * bits 16.. = mask of the failing columns */
#define HMPC_CERT_FAILED 0x100

/* One tolerance per class.  An argument and not a constant: the defaults are the bounds the project's own records are held
 * to, but a VALID polished record can exceed 1e-8 -- the polish verifies rows on their unit form, and an inactive row of
 * large norm (cart-pole systems at N = 40: norms 51 and 273) shows a primal inequality of 1.5e-8 .. 1.1e-7 and a gap of
 * 1.9e-7 (tests/test_certificates.py); a caller with such rows widens `polished`. */
typedef struct hmpc_cert_tol { double polished, unpolished, infeasible, weak; } hmpc_cert_tol; /* NULL: 1e-8, 5e-6, 1e-6, 1e-6 */

/* Certifies B records.  x0, x0_stride, fix: as for hmpc_solve_batch (fix may be NULL for a problem without binaries);
 * records: all six members required, B rows each (e.g. what hmpc_solve_batch filled).  residuals: B x HMPC_CERT_COUNT.
 * Any problem hmpc_create admits can be certified: the matrices are staged in LDS where they fit and read in place where
 * they do not.  Host-pointer form: copies in, runs, copies out, returns when done. */
int hmpc_certify_batch(hmpc_handle *h, const double *x0, int32_t x0_stride, const int8_t *fix, int32_t B,
                       const hmpc_result *records, const hmpc_cert_tol *tol /* nullable */,
                       double *residuals /* B x HMPC_CERT_COUNT */, int32_t *verdict /* B, nullable */);
/* Device-pointer form: every pointer except tol is device memory; asynchronous on `stream`.  It allocates nothing, never
 * synchronises and uses no workspace of the handle (hmpc_create keeps a copy of the unscaled matrices on the device), so
 * hmpc_solve_batch_device followed by this call on the same stream certifies a frontier without a host round trip. */
int hmpc_certify_batch_device(hmpc_handle *h, const double *d_x0, int32_t x0_stride, const int8_t *d_fix, int32_t B,
                              const hmpc_result *d_records, const hmpc_cert_tol *tol /* nullable, host */,
                              double *d_residuals, int32_t *d_verdict /* nullable */, void *stream);

/* ---- Branching a batch of solved nodes (records -> children with their lower bounds) --------------------------
 * The step of a branch-and-bound round between two solves: the reference's brancher (warm_start_hmpc/controller.py:395-429
 * _brancher: a child's bound is its parent's objective plus the parent's multiplier of the bound the branch tightens) with its
 * branching rule (controller.py:13-44 branch_in_time) and the prune / incumbent / branch decision of
 * branch_and_bound.py:476-489, for B records at once on the device (csrc/hmpc_branch.hip; per-node arithmetic:
 * csrc/hmpc_branch.h).  Per node b, from its row of `fix`, its record and cutoff[b] (cutoff NULL: +inf):
 *   pos        1 + the largest j with fix[j] >= 0, 0 if there is none: the binary branch_in_time fixes next, for ANY
 *              identifier, not only chronological prefixes; pos == T*nub: every binary is fixed
 *   child_lb2  [0] = obj + nu_ub[pos] (the 0-branch), [1] = obj + nu_lb[pos] (the 1-branch): one float64 addition each;
 *              both +inf when pos == T*nub or the node is not OPTIMAL
 *   word       exactly one of HMPC_BRANCH_BRANCHED / _COMPLETE / _PRUNED / _INFEASIBLE / _FAILED, and the flags below.
 *              obj is compared as `obj < cutoff`: a NaN objective (or cutoff) compares false and ends as PRUNED, never
 *              as BRANCHED or COMPLETE
 *   bits       ceil(T*nub / 64) words: bit j = the relaxed binary j of the primal row > 0.5 (NaN: 0) -- the rounding the
 *              fleet's dive prediction uses; only for a VERTEX node with pos < T*nub, zero otherwise
 * Children: the nodes flagged BRANCHED have two each, 0-branch first, in the order of the batch -- child_offset[b] is the
 * exclusive prefix sum of (2 if BRANCHED else 0), n_children[0] its total; rows child_offset[b] + v of
 *   child_fix     the parent's identifier with fix[pos] = v
 *   child_lb      child_lb2[v]
 *   child_parent  b
 *   child_warm    warm_base + b if the parent is a VERTEX (its record may be handed down: ready to be hmpc_warm.index of
 *                 the next solve, whose rows are the records of this batch from row warm_base on), else -1
 * Rows of the child arrays at and beyond n_children are not written.  mark_weak != 0: records->dual_obj[b] of a node with
 * HMPC_ITERS_WEAK becomes -inf (the node prunes at this step only: the warm-start shift then reopens the leaf whatever the
 * model error, controller.py:555-558); no other entry of the records is written.
 * records: obj, status, iters required; dual where child_lb2 or child_lb is asked for, primal where bits is, dual_obj
 * where mark_weak is set.  A problem without binaries has nothing to branch on: HMPC_EINVAL.  B == 0: HMPC_OK, nothing touched. */
#define HMPC_BRANCH_BRANCHED    0x01  /* OPTIMAL, obj < cutoff, pos < T*nub: two children */
#define HMPC_BRANCH_COMPLETE    0x02  /* OPTIMAL, obj < cutoff, pos == T*nub: an incumbent candidate */
#define HMPC_BRANCH_PRUNED      0x04  /* OPTIMAL, not (obj < cutoff) */
#define HMPC_BRANCH_INFEASIBLE  0x08  /* status HMPC_INFEASIBLE */
#define HMPC_BRANCH_FAILED      0x10  /* status > HMPC_INFEASIBLE: the record must not be used */
#define HMPC_BRANCH_VERTEX      0x100 /* OPTIMAL and HMPC_ITERS_POLISHED: the record may be handed down */
#define HMPC_BRANCH_WEAK        0x200 /* HMPC_ITERS_WEAK */
#define HMPC_BRANCH_UNCERTIFIED 0x400 /* HMPC_ITERS_UNCERTIFIED */
#define HMPC_BRANCH_HANDED      0x800 /* HMPC_ITERS_HANDED */
typedef struct hmpc_branch_out {  /* any member may be NULL (not wanted) */
    double   *obj;          /* B : copy of records->obj                                     */
    int32_t  *word, *pos;   /* B, B                                                         */
    double   *child_lb2;    /* B x 2                                                        */
    uint64_t *bits;         /* B x ceil(T*nub/64)                                           */
    int32_t  *child_offset; /* B : required if any child_* is set                           */
    int32_t  *n_children;   /* 1                                                            */
    int8_t   *child_fix;    /* 2B x T*nub                                                   */
    double   *child_lb;     /* 2B                                                           */
    int32_t  *child_parent; /* 2B                                                           */
    int32_t  *child_warm;   /* 2B                                                           */
} hmpc_branch_out;
/* Host-pointer form: copies in, runs, copies out (the child arrays up to n_children; records->dual_obj when mark_weak is
 * set), returns when done.  Replaces B calls of controller.py:395-429. */
int hmpc_branch_batch(hmpc_handle *h, const int8_t *fix, int32_t B, const hmpc_result *records, const double *cutoff /* nullable */,
                      int32_t warm_base, int32_t mark_weak, const hmpc_branch_out *out);
/* Device-pointer form: every pointer (and every member of d_records and d_out) is device memory; asynchronous on `stream`.
 * Up to three launches (digest, offsets, children), no allocation, no synchronisation, no workspace of the handle: it is
 * legal between two hmpc_solve_batch_device calls on one stream, so that solve -> branch -> solve (controller.py:395-429
 * between two passes of branch_and_bound.py:462-489) runs without a row leaving HBM -- the caller reads back n_children
 * alone, to size the next launch. */
int hmpc_branch_batch_device(hmpc_handle *h, const int8_t *d_fix, int32_t B, const hmpc_result *d_records, const double *d_cutoff /* nullable */,
                             int32_t warm_base, int32_t mark_weak, const hmpc_branch_out *d_out, void *stream);

/* ---- Closed loops in lockstep ("fleet") ---------------------------------------------------------------
 * K independent closed loops of the controller advanced together -- the shape of the reference's Monte-Carlo
 * study (notebooks/cart_pole_with_walls/statistical_analysis.py:93-196: per step one warm-started branch and
 * bound, branch_and_bound.py:408-499 + controller.py:395-429, then construct_warm_start, controller.py:431-564).
 * The trees live behind the handle: topology and bounds on the host, every multiplier row in HBM (written by
 * the QP kernel, referenced by index, shifted in place by the shift kernel); one call per MPC step, the rounds
 * of all trees share kernel launches.  Needs hmpc_set_shift_maps.  Per loop and step:
 *     hmpc_fleet_solve : MIQP from x0[k] by branch and bound started from the loop's current tree (its root for a
 *                        cold loop), `width` candidates per tree and round (1 = the reference's node order);
 *                        speculation = k > 0: descendants through the next k binaries ride in the launch of a
 *                        node and are consumed only if the search gets there (same result, fewer launches);
 *                        speculation < 0: dive prediction -- with a node whose parent's record is at hand, the rest of
 *                        the dive predicted from the parent's rounded relaxed binaries and the sibling of every step
 *                        ride along (2 (T nub - depth) nodes; for few loops: a cold start in a handful of launches);
 *                        cost[k] (+inf: infeasible, the loop stops), u0[k] (nu: applied input), x1[k] (nx: the
 *                        model's next state A x0 + B u0), solves[k], leaves[k]
 *     hmpc_fleet_shift : the tree becomes the warm start of the next step given the model error e0[k] of the step
 *                        (next state = x1 + e0); cover[k] nodes, reopened[k] of them lost their infeasibility proof
 * Any output pointer may be NULL.  hmpc_fleet_reset(f, k) makes loop k (-1: all) cold again.  A call that fails midway
 * (device error, a consumed node that did not converge) leaves some trees advanced and others not: the fleet then refuses
 * further steps until hmpc_fleet_reset(f, -1). */
typedef struct hmpc_fleet hmpc_fleet;
int hmpc_fleet_create(hmpc_handle *h, int32_t K, hmpc_fleet **out);
int hmpc_fleet_destroy(hmpc_fleet *f);
int hmpc_fleet_reset(hmpc_fleet *f, int32_t k);
/* Loop k has ended: its tree is dropped, it takes no part in further steps (no launches, no pool rows) until it is reset. */
int hmpc_fleet_stop(hmpc_fleet *f, int32_t k);
/* Rows of the multiplier pools in use / allocated.  Rows nobody references are reclaimed: hmpc_fleet_shift compacts, and
 * hmpc_fleet_solve starts the pools from zero when every tree is cold. */
int hmpc_fleet_rows(const hmpc_fleet *f, int64_t *used, int64_t *capacity);
int hmpc_fleet_solve(hmpc_fleet *f, const double *x0 /* K x nx */, int32_t width, int32_t speculation, double tol, double *cost,
                     double *u0, double *x1, int32_t *solves, int32_t *leaves);
int hmpc_fleet_shift(hmpc_fleet *f, const double *e0 /* K x nx */, int32_t *cover, int32_t *reopened);
/* kernel launches (rounds) and nodes sent to the QP kernel since creation */
int hmpc_fleet_stats(const hmpc_fleet *f, int64_t *rounds, int64_t *launched);
/* Nodes the fleet's searches pruned WITHOUT a certificate (HMPC_ITERS_UNCERTIFIED), and how many searches ended with such a
 * node whose bound before its solve lay below the final incumbent (or with no incumbent): there the returned optimum rests on
 * that prune.  Since creation. */
int hmpc_fleet_uncertified(const hmpc_fleet *f, int64_t *pruned, int64_t *searches_resting_on_one);
/* Parent -> child hand-down inside the fleet's searches (hmpc_warm; on by default): a child that is solved in a later
 * round than its parent receives the parent's record, which already lies in the fleet's HBM pools.  enable: 1 / 0, < 0:
 * leave as is.  verified (nullable): solves since creation whose handed-down active set verified. */
int hmpc_fleet_handdown(hmpc_fleet *f, int32_t enable, int64_t *verified);
/* Digest of a round on the device (off by default): the digest kernel of the branching entries above runs behind the QP
 * kernel on the fleet's stream, and a round copies back ONE block of objective, word, pos, the two child bounds and -- with
 * dive prediction -- the rounded binaries per node (32 + 8 ceil(T nub / 64) bytes) in place of objective, status, iters, a
 * strided row of 2 T nub multipliers and, with dive prediction, the whole primal row; the dual objective of a weak node is
 * set to -inf by the kernel and not by one blocking copy per node.  The tree stays on the host: selection, consumption order
 * and every result are those of the default path, bit for bit (controller.py:395-429 on the device, branch_and_bound.py:
 * 476-489 on the host).  enable: 1 / 0, < 0: leave as is. */
int hmpc_fleet_digest(hmpc_fleet *f, int32_t enable);
/* Host wall time of the fleet's calls by phase since creation (5 doubles, seconds): candidate selection, staging of the
 * rounds' nodes, device (copies, kernel, synchronisation), consumption of the results, node shifts. */
int hmpc_fleet_timing(const hmpc_fleet *f, double *seconds5);

/* ---- Incumbent exchange between the GPUs of a node (RCCL over xGMI) ----------------------------------
 * A frontier is sharded by node (node k to rank k mod nranks; nodes are independent, no data-path collective).
 * Once per branch-and-bound round every rank calls hmpc_allreduce_incumbent with its best upper bound and its
 * number of open candidates; on return *ub is the global best (every rank prunes against it) and *open the
 * largest count on any rank (zero exactly when all ranks are done: they stop in the same round).  One all-reduce
 * (MIN) of two float64.  Setup as for any RCCL communicator: rank 0 calls hmpc_comm_unique_id and hands the
 * 128 bytes to the other ranks (the caller's transport), then every rank calls hmpc_comm_create.  RCCL is
 * loaded at run time; a process that never creates a communicator does not need it.
 * A rank whose own search failed still owes the others the round they are waiting in: it calls once more with
 * *ub = -INFINITY, and every rank that receives -INFINITY stops with an error of its own (the convention of
 * warm_start_hmpc_amd/distributed.py: IncumbentExchange.abort / PeerFailure). */
typedef struct hmpc_comm hmpc_comm;
int hmpc_comm_unique_id(void *id128 /* 128 bytes out */);
int hmpc_comm_create(hmpc_handle *h, int32_t nranks, int32_t rank, const void *id128, hmpc_comm **out);
int hmpc_allreduce_incumbent(hmpc_comm *c, double *ub /* in/out */, int32_t *open /* in/out */);
/* The same exchange on device memory and on the caller's stream: pair_device[0] = upper bound, pair_device[1] =
 * -(open candidates), reduced in place (MIN); enqueued, not waited for -- work launched on `stream` afterwards sees the
 * global pair.  `stream` is a hipStream_t (NULL: the default stream). */
int hmpc_allreduce_incumbent_device(hmpc_comm *c, double *pair_device /* 2 doubles, in/out */, void *stream);
/* After the last round (once per search; every rank calls it): which rank owns the global incumbent, and its binary
 * assignment on every rank.  In: *ub this rank's best upper bound (+INFINITY: none), assignment its incumbent's nbytes
 * bytes (T*nub binaries for this solver; ignored on ranks that do not own the winner).  Out: *ub the global best, *owner
 * the lowest rank that holds it (-1: no rank has an incumbent, the MIQP is infeasible; assignment untouched), assignment
 * the owner's bytes on every rank (one ncclBroadcast).  SURVEY.md 8(b)/(e).
 * nbytes <= T*nub of the handle the communicator was created on.  A bound of -INFINITY or NaN on any rank (the abort
 * convention above) makes EVERY rank return HMPC_EINVAL after the first reduction; any other failure between the
 * collectives aborts the communicator (the peers are already waiting in the next one). */
int hmpc_publish_incumbent(hmpc_comm *c, double *ub /* in/out */, int8_t *assignment /* in/out */, int32_t nbytes, int32_t *owner);
int hmpc_comm_destroy(hmpc_comm *c);

/* ---- batched dense LPs of the offline terminal ingredients ----
 *
 *     maximise c_k'x   subject to   A x <= b_k (+ 1 on row relax[k]),   x in R^n free,   k = 0 .. B-1
 *
 * One launch replaces one sweep of the reference's one-Gurobi-LP-at-a-time loops:
 *   warm_start_hmpc/mcais.py:103-118       A = D_inf, c_k = (D A^t)_k, b = e_inf shared          (one sweep per horizon t)
 *   warm_start_hmpc/mcais.py:169-182       A = E, c_k = E_k, b = f shared, relax[k] = k         (redundant facets)
 *   warm_start_hmpc/controller.py:205-226  A = [F G], c_k = row k of [F_Tm1 G_Tm1], b = h shared; column k of the
 *                                          multiplier map M is z[k] (the reference states the dual LP
 *                                          min h'mu s.t. [F G]'mu = c_k, mu >= 0; HMPC_UNBOUNDED here is its "infeasible")
 * Host arrays, row-major: A[m][n]; c[B][n] with c_stride = n, or one c[n] with c_stride = 0; b likewise with b_stride =
 * m or 0; relax[B] or NULL (entries -1: none).  device < 0: the current device.  tol <= 0, max_iter <= 0: defaults
 * (1e-9, 100).  Out: obj[B] = c_k'x (NaN unless optimal), x[B][n], z[B][m] >= 0 or NULL (A'z = c_k at an optimum; a
 * Farkas ray A'z = 0, b'z < 0 when the set is empty), status[B] in {HMPC_OPTIMAL, HMPC_INFEASIBLE (empty set),
 * HMPC_UNBOUNDED, HMPC_MAXITER, HMPC_NUMERICAL}, iters[B].  Limits: n <= 64; the row vectors of one LP must fit one
 * CU's LDS (m <~ 1800).  Values of an optimum are exact to rounding (the interior-point iterate is moved to the
 * vertex), so the reference's comparisons with 0 (mcais.py:128) and 1e-7 (mcais.py:181) see what a simplex code shows. */
int hmpc_lp_solve_batch(int32_t device, int32_t n, int32_t m, const double *A, const double *c, int32_t c_stride,
                        const double *b, int32_t b_stride, const int32_t *relax, int32_t B, double tol, int32_t max_iter,
                        double *obj, double *x, double *z, int32_t *status, int32_t *iters);

/* Kernels compiled with the problem's sizes.  The reference takes any MLDSystem at one speed (warm_start_hmpc/controller.py:58-117).
 * hmpc_create compiles the kernel of each wave count (1 / 2 / 4 waves per node) ONCE MORE for the problem it is given, from the
 * sources next to the library, with the offline compiler (a child process), its integer sizes as constants of the translation
 * unit, into an on-disk cache (csrc/hmpc_jit.h: environment HMPC_JIT / HMPC_JIT_SIZED / HMPC_JIT_CACHE / HMPC_HIPCC): the
 * register kernel (static row map: rows and recursions in registers) where the problem admits it -- nx + nu <= 16, every
 * [F G] row with at most two input coefficients, columns of at most 16 entries, at most 128 Gram entries with terms, at least
 * one binary --, the run-time-sized kernel or, beyond one CU's LDS, its streaming form elsewhere.  Same source, same code
 * paths, same feature set as the shipped kernels, which serve wherever the compilation is not possible (no compiler, no
 * sources, HMPC_JIT=0 / HMPC_JIT_SIZED=0): the built-in register kernels of the two cart-pole shapes, the run-time-sized kernel
 * for every other system.
 * Two nets around code nobody has run before (the reference never hands back an undecided node, bounded_qp.py:216-228):
 *   first-use check : the first launch through a wave count solves 64 nodes -- spread over its batch, plus the root relaxation
 *                      and the deepest node -- with the compiled and the shipped kernel and compares statuses and objectives;
 *                      a kernel that disagrees is dropped for the handle (message on stderr).  One stream synchronisation per
 *                      wave count, inside that solve call -- or ahead of time through hmpc_validate_kernels (callers that
 *                      capture their stream or must not block).  HMPC_JIT_SELFCHECK=0 switches both nets off.
 *   second opinion  : in EVERY solve call (hmpc_solve_batch, hmpc_solve_batch_device, hmpc_fleet_solve) the nodes a compiled
 *                      kernel leaves MAXITER / NUMERICAL are listed on the device and solved again by the shipped kernel in
 *                      the same stream, without synchronisation; its records replace theirs.  A compiled kernel that leaves
 *                      nodes undecided which the shipped kernel decides is dropped when the counts arrive (the next call, or
 *                      hmpc_second_opinion_review after the caller has synchronised).
 *   hmpc_kernel_info : which kernel serves the problem for 1 / 2 / 4 waves per node: 0 run-time-sized, 1 its streaming
 *                      form, 2 built-in register kernel, 4 / 5 / 6 the run-time-sized kernel / its streaming form / the register
 *                      kernel compiled with this problem's sizes.
 *   hmpc_kernel_recipe : 1 per wave count whose compiled kernel was built with the compiler's ILP schedule (8 - 15 % faster; only
 *                      binaries listed in the cache's VALIDATED manifest, which tests/gpu_validate_ilp.py writes after running each of
 *                      them against the oracle: that schedule produced most of the wrong binaries of rounds 4 and 5), 0: the
 *                      compiler's default schedule -- the recipe of every kernel compiled for a problem nobody has validated.
 *   hmpc_jit_stats   : compiled kernels dropped by the nets; solve calls with a second opinion; batches on which it agreed.
 *   hmpc_jit_build_problem : everything hmpc_create would compile for this problem, ahead of time and without a GPU (the host
 *                      side of hmpc_create, nothing uploaded); paths: the shared objects, newline separated (may be NULL). */
int hmpc_kernel_info(const hmpc_handle *h, int32_t *kind3);
int hmpc_kernel_recipe(const hmpc_handle *h, int32_t *ilp3);
int hmpc_jit_stats(const hmpc_handle *h, int32_t *dropped, int32_t *second_runs, int32_t *second_agreed);
int hmpc_jit_build_problem(const hmpc_problem *problem, const hmpc_options *options, char *paths, int32_t paths_len);
int hmpc_validate_kernels(hmpc_handle *h, const double *d_x0, int32_t x0_stride, const int8_t *d_fix, int32_t B, void *stream);
int hmpc_second_opinion_review(hmpc_handle *h);

/* Number of workgroups the last launch used, and LDS bytes per workgroup (for reports). */
int hmpc_launch_info(const hmpc_handle *h, int32_t *grid, int32_t *lds_bytes);

/* Text of the last error on this thread ("" if none). */
const char *hmpc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HMPC_H */
