/*
 * hmpc_search.h -- K branch-and-bound searches whose trees live on the device.
 *
 * include/hmpc.h solves, certifies and branches a frontier through device pointers; what was left to the caller is the search
 * around those calls: which nodes of a tree go next, the incumbent, the tree itself (the reference's loop,
 * warm_start_hmpc/branch_and_bound.py:462-489; here tree_select / tree_consume of csrc/hmpc_tree.h and _Tree of
 * warm_start_hmpc_amd/batched.py, both on the host).  An hmpc_search keeps K independent trees in HBM and advances them in
 * lockstep, at most one QP launch per round; the host reads back one small word per round, the size of the next launch.
 *
 * Per tree the semantics are tree_select + tree_consume without dive prediction and -- at the default depth 0 -- without speculation:
 *   select   candidates are the nodes with alive && lb < ub - tol; the `width` smallest by (lb, index) are picked, in that
 *            order (first wins ties; +inf bounds are never picked).  A tree without candidates gets HMPC_SEARCH_DONE, and
 *            HMPC_SEARCH_INCUMBENT with it if it has an incumbent.  Only trees whose state word is 0 take part.
 *   consume  pick by pick in selection order, SERIALLY within a tree -- a COMPLETE pick lowers ub and the next pick of the
 *            same round is compared with the new cutoff.  Node i with record row r:
 *              status > HMPC_INFEASIBLE: the tree gets HMPC_SEARCH_FAILED and stops; this and its later picks are not consumed
 *              word = the decision of hmpc_branch_batch for (record, cutoff ub - tol) (csrc/hmpc_branch.h)
 *              BRANCHED with n + 2 > node_cap: the tree gets HMPC_SEARCH_OVERFLOW and stops, nothing of the pick is written
 *              solves++; HMPC_ITERS_UNCERTIFIED: uncertified++, unc_lb = min(unc_lb, lb[i]) (the bound BEFORE the solve)
 *              lb[i] = obj, row[i] = r; HMPC_ITERS_WEAK: dual_obj[r] = -inf (the shift then reopens the leaf)
 *              PRUNED / INFEASIBLE: the node stays a leaf;  COMPLETE: ub = obj, the node is the incumbent
 *              BRANCHED: two children are appended, 0-branch first: bound obj + multiplier of the tightened bound, they carry
 *              row r, and hand row r down if the parent is a VERTEX; the node is no leaf any more
 * State: every tree owns a slab of node_cap nodes (identifier, bound, row, row to hand down, alive), so that list order is
 * index order; one pool of row_cap record rows in the layout of hmpc_result holds every solved node; a round's records are
 * rows row0 .. row0 + B - 1, and row0 advances by B with every consumed round.
 * The search uses the handle's workspaces through the solve call: at most ONE launch per handle may be in flight.
 *
 * Speculation (hmpc_search_set_speculation, depth s in 0 .. 4, default 0: everything above, bit for bit) is tree_expand of
 * csrc/hmpc_tree.h without dive prediction: a launch of a few nodes costs a node's latency whatever it carries, so every picked
 * node that has to be launched rides with ALL its descendants through its next s free binaries; their records wait in the pool,
 * and a later pick of such a descendant is consumed from its waiting record without a launch.
 * With S(L) = 2^(L+1) - 1 and pos(i) = the number of leading entries of node i's identifier up to its last fixed one, every node
 * carries two more fields: srow, the pool row of its own waiting record or -1, and sleft, the levels of waiting descendants below
 * that record.  begin, advance and a branch without waiting descendants set them to -1 and 0.
 *   select   picks exactly as above -- speculation never changes which nodes a round picks.  A pick with srow[i] >= 0 emits no
 *            row.  Any other pick emits a block of S(L) rows, L = min(s, T nub - pos(i)), in PRE-ORDER: row r is the node, row
 *            r + 1 opens the 0-child's block of S(L-1) rows, row r + 1 + S(L-1) the 1-child's; row r + q carries the node's
 *            identifier with the binaries at pos, pos + 1, ... set along the path that pre-order index q names.  Blocks lie tree
 *            by tree and in pick order within a tree; B is the number of emitted rows, and row0 + B > row_cap is HMPC_ETOOBIG
 *            with nothing changed.  Of the staged round a block's first row receives the row handed down to its node and carries
 *            (tree, node); the descendants receive -1 (their parent rides in the same launch) and carry (tree, -1).
 *   consume  a pick with srow[i] >= 0 uses r = srow[i], L = sleft[i]; a launched pick its block's first row and the L of select.
 *            Then everything above happens with (i, r), the refusals included (a refused pick writes nothing, the two fields
 *            neither), and: srow[i] = -1; child v of a BRANCHED node gets srow = r + 1 + v S(L-1), sleft = L - 1 if L > 0, else
 *            -1 and 0.  The children still hand row r down: it is used once a child without waiting descendants has children of
 *            its own to launch.  A waiting record with status > HMPC_INFEASIBLE fails its tree WHEN IT IS CONSUMED, never
 *            before; waiting records that are never consumed change nothing, and begin and advance drop them.
 * With s > 0 a round may have picks and no launch (every pick's record waits): B == 0 no longer says that every tree has
 * stopped -- the number of picks P does (hmpc_search_staged), and it comes back in the round's one readback.
 * The invariant: with hand-down off a record is a function of (x0, identifier) alone, so for any s every round's picks and every
 * tree after every round equal those at s = 0 in every field but pool row numbers (row, wrow, inc_row) and srow / sleft; the
 * records those row numbers point at are bit-equal; only the number of QP launches falls.  With hand-down ON this does not hold
 * bit for bit: speculated descendants are solved cold, where at s = 0 they would have received their parent's record.
 * A step needs up to S(s) pool rows per launched pick instead of one.
 */
#ifndef HMPC_SEARCH_H
#define HMPC_SEARCH_H

#include "hmpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* state word of a tree (0: running) */
#define HMPC_SEARCH_DONE 0x1      /* no candidate left */
#define HMPC_SEARCH_INCUMBENT 0x2 /* ... and it has an incumbent */
#define HMPC_SEARCH_FAILED 0x4    /* a consumed node ended MAXITER / NUMERICAL */
#define HMPC_SEARCH_OVERFLOW 0x8  /* node_cap */

typedef struct hmpc_search hmpc_search;

/* K trees of node_cap nodes each and one pool of row_cap record rows.  HMPC_EINVAL without touching the GPU: null handle or
 * out, K, node_cap or row_cap <= 0, a problem without binaries. */
int hmpc_search_create(hmpc_handle *h, int32_t K, int32_t node_cap, int32_t row_cap, hmpc_search **out);
int hmpc_search_destroy(hmpc_search *s);

/* A step begins: x0 (K x nx, host).
 * count == NULL: every tree is its root (lb = -inf).
 * Else tree k starts from count[k] leaves, tree by tree: fix (sum x T*nub), lb (sum), and -- where dual != NULL -- their
 * dual rows (sum x n_dual) and dual objectives (sum), which take the first rows of the pool (leaf j carries row j; nothing
 * is handed down to it).  A tree with count[k] == 0 has nothing to search: it ends DONE at the first select.
 * The pool and all counters start from zero.  HMPC_EINVAL: count[k] < 0 or > node_cap, sum(count) beyond the pool with dual. */
int hmpc_search_begin(hmpc_search *s, const double *x0, const int32_t *count, const int8_t *fix, const double *lb,
                      const double *dual, const double *dual_obj);

/* One round in two halves, for callers that solve elsewhere and for the tests.
 * select stages the round and returns its size in *B: the one synchronisation of a round.  width in 1 .. 64.
 * B = 0: every tree has stopped (at speculation depth 0; else see hmpc_search_staged).
 * row0 + B > row_cap: HMPC_ETOOBIG with nothing changed. */
int hmpc_search_select(hmpc_search *s, int32_t width, double tol, int32_t handdown, int32_t *B, void *stream);

/* Device pointers of the staged round (any pointer NULL: not wanted): B rows of x0 (stride nx) and of identifiers,
 * the hand-down ready for hmpc_solve_batch_device (rows = the pool's; index[b] = the row node b receives if hand-down was on
 * at select, else -1), d_rows: the members point at row row0 of the pool, so that hmpc_solve_batch_device writes the records
 * where consume reads them. */
int hmpc_search_batch(const hmpc_search *s, const double **d_x0, const int8_t **d_fix, hmpc_warm *d_warm,
                      hmpc_result *d_rows, int32_t *row0);

/* Host records into the rows of the staged round (an outside solver; the tests' synthetic records).  B: the staged size;
 * obj, status, iters required, the other members are copied where given. */
int hmpc_search_put_records(hmpc_search *s, int32_t B, const hmpc_result *host_records);

/* Consumes the staged round.  Asynchronous on `stream`.  HMPC_EINVAL without a staged round (one without a pick). */
int hmpc_search_consume(hmpc_search *s, double tol, void *stream);

/* select -> hmpc_solve_batch_device -> consume until no tree has a pick or max_rounds (<= 0: none).  rounds, launched
 * (nullable): rounds and nodes of this call; at speculation depth 0 every round is one QP launch, else a round whose picks all
 * have waiting records skips the solve and still consumes (hmpc_search_counters tells the two apart).  One synchronisation per
 * round either way.  The states of the trees say how each of them ended (hmpc_search_results). */
int hmpc_search_run(hmpc_search *s, int32_t width, double tol, int32_t handdown, int32_t max_rounds, void *stream,
                    int32_t *rounds, int64_t *launched);

/* Per tree, any pointer NULL.
 * cost: +inf without incumbent.
 * u0 (nu), x1 (nx): from the incumbent's primal row, NaN without one.  binaries: the incumbent's identifier, -1 without one.
 * leaves: alive nodes. */
int hmpc_search_results(hmpc_search *s, double *cost, double *u0, double *x1, int8_t *binaries /* K x T*nub */,
                        int32_t *solves, int32_t *leaves, int32_t *state, int32_t *uncertified);

/* The alive nodes of all trees, tree by tree in list order -- the inputs of hmpc_shift_batch.
 * owner, fix, lb; dual and dual_obj are gathered through `row` (zeros where row < 0).
 * has_dual: 0 where row < 0.
 * n: capacity in / count out (HMPC_ETOOBIG with the count in *n when the capacity is short; nothing else is written).
 * Any of the arrays may be NULL. */
int hmpc_search_leaves(hmpc_search *s, int32_t *n, int32_t *owner, int8_t *fix, double *lb, double *dual,
                       double *dual_obj, uint8_t *has_dual);

/* The step that ended becomes the cover of the next one, on the device (the reference's construct_warm_start,
 * controller.py:431-564, for all K trees): retain -> shift -> adopt, then the state of a fresh hmpc_search_begin.
 * e0 (K x nx, host; NULL: zeros): the model error of the step.  x0_next (K x nx, host; NULL: x1 + e0 from the incumbent's row).
 * cover, reopened (K each, host, nullable): leaves tree k carries over / how many of them carry no usable bound.
 * Requires hmpc_set_shift_maps, a begun step and no staged round.
 * A tree advances if and only if its state is exactly DONE | INCUMBENT; every other tree gets an empty cover (and, without
 * x0_next, keeps its x0).  Of an advancing tree the alive nodes whose stage-0 binaries are free or those of the incumbent's
 * input (rounded) are kept, in list order; kept leaf j of tree k becomes node j, with the shifted identifier, the shifted bound
 * and row first[k] + j of the pool, whose rows 0 .. B - 1 are the shifted dual rows (B: all kept leaves; the next round's
 * records begin at row B).  A leaf that carried no row shifts from a row of zeros and counts as reopened.
 * A tree one of whose kept leaves the shift kernel dropped -- the two disagree on the retain rule -- begins the next step
 * HMPC_SEARCH_FAILED.
 * HMPC_EINVAL: a tree is still running (state 0).  HMPC_ETOOBIG: B > row_cap.  Either way nothing has changed.
 * One readback (12 bytes) is the only synchronisation when cover and reopened are NULL. */
int hmpc_search_advance(hmpc_search *s, const double *e0, const double *x0_next, int32_t *cover, int32_t *reopened, void *stream);

/* The trees as they stand are carried to a neighbouring initial state of the SAME stage, on the device: x0_new (K x nx, host).
 * x0 enters a node's QP only through the right-hand side of x_0 = x0, so every record's multipliers stay dual feasible at any
 * x0 and its dual (or Farkas) objective moves by exactly -lam_0 . (x0_new - x0), lam_0 the first nx entries of its dual row
 * (the run-time half of the reference's construct_warm_start, controller.py:541-558, without the time shift).  A search solved
 * for the PREDICTED next state while the plant moves is thereby a complete proof tree for the measured one, bounds moved by
 * O(|x0_new - x0|): advance(e0 = NULL) -> run [idle time] -> rebase(measured state) -> run.
 * cover, reopened (K each, host, nullable): leaves tree k keeps / how many of them carry no usable bound.
 * Requires a begun step and no staged round; hmpc_set_shift_maps is NOT needed.
 * A tree takes part if and only if its state has neither FAILED nor OVERFLOW -- a RUNNING tree (state 0) does: the search need
 * not have ended.  Every other tree becomes its root at the new state, as hmpc_search_begin with count == NULL leaves it
 * (cover 0, reopened 0).  Of a tree that takes part ALL alive nodes are kept, in list order; kept leaf j of tree k becomes node
 * j with its identifier unchanged and row first[k] + j of the pool, whose rows 0 .. B - 1 are verbatim copies of the dual rows
 * the leaves carried (B: all kept leaves; the pools swap as in an advance, so the pool is compacted and the next round's records
 * begin at row B); a node without a row (row < 0) gets the row of zeros and counts as reopened.  With r the row a leaf carried,
 * delta = x0_new[k] - x0[k], and every product and sum rounded on its own (no fma), j = 0 .. nx - 1 in order:
 *   dot = sum_j dual[r][j] * delta[j];  obj = max(dual_obj[r] - dot, 0);  the new row's dual_obj = obj
 *   lb not infinite: lb' = obj;   lb infinite and obj <= 0: lb' = 0, reopened;   lb infinite and obj > 0: lb' = lb
 * (the tail of both shift kernels, isinf and all; a weak record, dual_obj = -inf, reopens an infeasible leaf).
 * Nothing is handed down across a re-base (wrow = -1) and waiting speculative records are dropped (srow = -1, sleft = 0).
 * Every tree then has the scalars of a fresh begin -- ub = +inf, no incumbent, state 0, solves and uncertified 0 --, the counters
 * of hmpc_search_counters start from zero, and x0 = x0_new.
 * HMPC_EINVAL without touching the GPU: null search or x0_new.  HMPC_ETOOBIG: B > row_cap, with nothing changed.
 * One readback (12 bytes) is the only synchronisation when cover and reopened are NULL. */
int hmpc_search_rebase(hmpc_search *s, const double *x0_new, int32_t *cover, int32_t *reopened, void *stream);

/* Host copies, for a caller that solves the staged round elsewhere and for inspection (each synchronises; any array NULL).
 * get_batch: the staged round (B: its size) -- x0 (B x nx), fix (B x T*nub), the rows handed down, and the (tree, node) of
 *   every pick.
 * tree: tree k as it stands.  scalars6: n, inc, inc_row, solves, uncertified, state; bounds2: ub, unc_lb; the whole slab,
 *   node_cap entries each (entries at and beyond n are whatever earlier steps left).
 * rows: rows first .. first + count - 1 of the pool into (write == 0) or from (write != 0) the host arrays of `host`. */
int hmpc_search_get_batch(hmpc_search *s, int32_t B, double *x0, int8_t *fix, int32_t *warm, int32_t *tree, int32_t *node);
int hmpc_search_tree(hmpc_search *s, int32_t k, int32_t *scalars6, double *bounds2, int8_t *fix, double *lb, int32_t *row,
                     int32_t *wrow, uint8_t *alive);
int hmpc_search_rows(hmpc_search *s, int32_t first, int32_t count, const hmpc_result *host, int32_t write);

/* Speculation depth of the rounds to come (see the top of this file), 0 .. 4; a new search has 0.  Regrows the staging of a
 * round to min(K 64 S(depth), row_cap) rows, so that select never allocates.  HMPC_EINVAL: depth outside 0 .. 4 (checked first,
 * without touching the GPU), a staged round, K 64 S(depth) beyond int32.  Waiting records of an earlier depth stay valid. */
int hmpc_search_set_speculation(hmpc_search *s, int32_t depth);

/* The staged round as the host knows it from select's readback, without a synchronisation: its picks (0: none is staged, the
 * search has stopped) and its rows B.  Either pointer may be NULL. */
int hmpc_search_staged(const hmpc_search *s, int32_t *picks, int32_t *B);

/* out[4], all since hmpc_search_begin: rounds consumed, QP launches among them (rounds with B > 0), rows launched (the sum of B),
 * picks whose record was waiting when their round was staged. */
int hmpc_search_counters(const hmpc_search *s, int64_t *out);

/* srow and sleft of tree k's slab, node_cap entries each (synchronises; either array NULL). */
int hmpc_search_tree_waiting(hmpc_search *s, int32_t k, int32_t *srow, int32_t *sleft);

#ifdef __cplusplus
}
#endif
#endif /* HMPC_SEARCH_H */
