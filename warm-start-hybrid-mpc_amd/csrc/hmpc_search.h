// hmpc_search.h -- what one tree of a device-resident search does in a round (include/hmpc_search.h), item by item.
//
// Plain inline functions that compile for the device (hipcc) and for the host (g++), as hmpc_branch.h does: which nodes are
// candidates and in which order they are picked, what consuming ONE pick does to its tree, and what the end of a step does to it
// (hmpc_search_advance: which leaves it keeps, what the shift is given for them, what adoption makes of the tree) or a move to a
// neighbouring initial state (hmpc_search_rebase: which trees take part, how a row's dual objective and a leaf's bound move).  Every decision
// about a record is a function of hmpc_branch.h (branch_word, branch_child_lb, branch_child_warm; pos from branch_pos_*): nothing
// of it is restated here.  The kernels (hmpc_search.hip) supply the workgroup argmin, the scan over the trees and the lane loops over
// identifier rows; tests/host/search_driver.cpp and advance_driver.cpp walk the same functions serially under AddressSanitizer.
//
// Semantics: tree_select / tree_consume of hmpc_tree.h without dive (reference: branch_and_bound.py:462-489), with the record's
// decision taken as hmpc_branch_batch takes it (`obj < cutoff`: a NaN objective prunes).  Speculation (tree_expand, dive = false)
// is the block arithmetic further down: a launched pick rides with its descendants through its next binaries, in pre-order, and a
// node knows the pool row of its own waiting record (srow) and how many levels of waiting descendants lie below it (sleft).
#ifndef HMPC_SEARCH_CORE_H
#define HMPC_SEARCH_CORE_H

#include "../../include/hmpc_search_anytime.h" // (includes hmpc_search.h)
#include "hmpc_branch.h"

#define SEARCH_MAX_WIDTH 64 // picks per tree and round at most: the stride of a tree's picks

// Everything of a search that lives in HBM, as views.  Slabs: tree k's node i is element k * node_cap + i.
struct SearchState {
    int K, node_cap, row_cap;
    int8_t *fix;                          // (K node_cap) x nfix
    double *lb;                           // K node_cap
    int32_t *row, *wrow;                  // K node_cap: pool row whose dual row the node carries / record row to hand down, or -1
    uint8_t *alive;                       // K node_cap
    int32_t *n, *inc, *inc_row, *solves, *uncertified, *state; // K each
    double *ub, *unc_lb, *x0;             // K, K, K x nx
    double *p_obj, *p_dual_obj;           // the pool: row_cap rows in the layout of hmpc_result
    int32_t *p_status, *p_iters;
    double *p_primal, *p_dual;
    int32_t *picks, *count, *offset;      // the staged round: K x SEARCH_MAX_WIDTH nodes in selection order, K, K (exclusive scan of count)
    int32_t *word;                        // [0] B  [1] a tree has stopped FAILED / OVERFLOW  [2] a node receives a record  [3] the round fits the pool  [4] picks  [5] picks whose record waits
    int8_t *b_fix;                        // the batch: B x nfix
    double *b_x0;                         // B x nx
    int32_t *b_warm, *b_tree, *b_node;    // B each
    // speculation (new members at the end: a state initialised without them has none -- srow == nullptr: no waiting records, depth 0)
    int32_t *srow, *sleft;                // K node_cap: pool row of the node's own waiting record or -1 / levels of waiting descendants below it
    int32_t *plev, *pfirst;               // the staged round, K x SEARCH_MAX_WIDTH: levels of a launched pick's block (-1: its record waits) / first row of the block within its tree's rows
    int spec;                             // speculation depth, 0 .. SEARCH_MAX_SPEC
    // anytime searches (include/hmpc_search_anytime.h; at the end again, and zeros mean rule 0 and no budget)
    int rule;                             // HMPC_RULE_*
    int budget1;                          // max_solves + 1; 0: no budget
    int32_t *open;                        // K: the staged round found the tree with candidates and no budget left (null: no budgets)
};

struct SearchTree { // one tree of it
    int8_t *fix;
    double *lb;
    int32_t *row, *wrow;
    uint8_t *alive;
    int32_t *n, *inc, *inc_row, *solves, *uncertified, *state;
    double *ub, *unc_lb;
    int32_t *srow, *sleft; // (null without speculation)
};

HMPC_HD SearchTree search_tree(const SearchState &s, int nfix, int k)
{
    const size_t o = (size_t)k * s.node_cap;
    return SearchTree{s.fix + o * nfix, s.lb + o, s.row + o, s.wrow + o, s.alive + o, s.n + k, s.inc + k, s.inc_row + k, s.solves + k,
                      s.uncertified + k, s.state + k, s.ub + k, s.unc_lb + k, s.srow ? s.srow + o : nullptr, s.srow ? s.sleft + o : nullptr};
}

// ---- select --------------------------------------------------------------------------------------------------------------------
HMPC_HD bool search_running(int32_t state) { return state == 0; }

// (a +inf bound is never below ub - tol, a NaN bound neither)
HMPC_HD bool search_candidate(uint8_t alive, double lb, double ub, double tol) { return alive && lb < ub - tol; }

// keys (lb, index), ordered by bound, then by index: first wins ties
HMPC_HD bool search_key_less(double la, int ia, double lb, int ib) { return la < lb || (la == lb && ia < ib); }

// The next pick after (plb, pi) -- (-inf, -1) before the first --: of candidates a and b (index < 0: none) the smaller key
// that lies after the last pick.  take(best, candidate): whether the candidate replaces the best so far.
HMPC_HD bool search_take(double blb, int bi, double l, int i, double plb, int pi)
{
    if (i < 0 || !search_key_less(plb, pi, l, i)) return false;
    return bi < 0 || search_key_less(l, i, blb, bi);
}

// serial form of one tree's selection; returns the number of picks (the kernel runs the same two functions over a workgroup)
HMPC_HD int search_select_serial(const SearchTree &t, int width, double tol, int32_t *picks)
{
    if (!search_running(*t.state)) return 0;
    const int n = *t.n;
    const double ub = *t.ub;
    double plb = -INFINITY;
    int pi = -1, cnt = 0;
    while (cnt < width) {
        double blb = 0.0;
        int bi = -1;
        for (int i = 0; i < n; i++)
            if (search_candidate(t.alive[i], t.lb[i], ub, tol) && search_take(blb, bi, t.lb[i], i, plb, pi)) { blb = t.lb[i]; bi = i; }
        if (bi < 0) break;
        picks[cnt++] = bi;
        plb = blb;
        pi = bi;
    }
    return cnt;
}

// state of a tree that has no candidate left
HMPC_HD int32_t search_done_word(int32_t inc) { return HMPC_SEARCH_DONE | (inc >= 0 ? HMPC_SEARCH_INCUMBENT : 0); }

// ---- anytime: the rule's order, the budgeted selection, the stop word, the bound of a tree (include/hmpc_search_anytime.h) --------
// All rules are ONE order over keys (first, index) under search_key_less / search_take: first = the bound (best-first), -index
// (depth-first: the largest index comes first) or index (breadth-first).  An index is exact as a double, and no key of the two
// index rules is -inf, the key before the first pick.
HMPC_HD int search_tree_rule(int rule, int32_t inc)
{
    if (rule != HMPC_RULE_DIVE_THEN_BEST) return rule;
    return inc < 0 ? HMPC_RULE_DEPTH_FIRST : HMPC_RULE_BEST_FIRST;
}

// (rule: what search_tree_rule returns -- one of the first three)
HMPC_HD double search_rule_key(int rule, double lb, int i)
{
    return rule == HMPC_RULE_DEPTH_FIRST ? -(double)i : rule == HMPC_RULE_BREADTH_FIRST ? (double)i : lb;
}

// picks a running tree may stage: min(width, max_solves - solves), width without a budget
HMPC_HD int search_pick_limit(int width, int budget1, int32_t solves)
{
    if (budget1 <= 0) return width;
    const int left = budget1 - 1 - solves;
    return left < 0 ? 0 : left < width ? left : width;
}

// Serial form of one tree's selection under a rule and a budget (the kernel runs the same functions over a workgroup).  With the
// budget exhausted ONE candidate is still looked for and none is picked: *open says whether the tree has candidates and no budget.
HMPC_HD int search_select_anytime(const SearchTree &t, int rule, int budget1, int width, double tol, int32_t *picks, int32_t *open)
{
    *open = 0;
    if (!search_running(*t.state)) return 0;
    const int n = *t.n, order = search_tree_rule(rule, *t.inc), limit = search_pick_limit(width, budget1, *t.solves);
    const int probe = limit > 0 ? limit : 1;
    const double ub = *t.ub;
    double pk = -INFINITY;
    int pi = -1, found = 0;
    while (found < probe) {
        double bk = 0.0;
        int bi = -1;
        for (int i = 0; i < n; i++) {
            const double key = search_rule_key(order, t.lb[i], i);
            if (search_candidate(t.alive[i], t.lb[i], ub, tol) && search_take(bk, bi, key, i, pk, pi)) { bk = key; bi = i; }
        }
        if (bi < 0) break;
        if (found < limit) picks[found] = bi;
        found++;
        pk = bk;
        pi = bi;
    }
    const int cnt = found < limit ? found : limit;
    *open = found > cnt;
    return cnt;
}

// state of a running tree that stages no pick: out of budget with candidates left, or done
HMPC_HD int32_t search_stop_word(int32_t inc, int32_t open)
{
    return open ? HMPC_SEARCH_BUDGET | (inc >= 0 ? HMPC_SEARCH_INCUMBENT : 0) : search_done_word(inc);
}

// hmpc_search_set_budget lets exactly these trees run again
HMPC_HD bool search_budget_stopped(int32_t state) { return (state & ~HMPC_SEARCH_INCUMBENT) == HMPC_SEARCH_BUDGET; }

// the smaller of two bounds; a NaN b is skipped (a is never NaN: it starts from +inf)
HMPC_HD double search_bound_min(double a, double b) { return b < a ? b : a; }

// serial form of what a tree proves: *lower = min(min over alive nodes of lb, unc_lb), *open = its candidates at tol
HMPC_HD void search_bounds_serial(const SearchTree &t, double tol, double *lower, int32_t *open)
{
    double lo = INFINITY;
    int32_t cand = 0;
    const double ub = *t.ub;
    for (int i = 0; i < *t.n; i++) {
        if (t.alive[i]) lo = search_bound_min(lo, t.lb[i]);
        cand += search_candidate(t.alive[i], t.lb[i], ub, tol);
    }
    *lower = search_bound_min(lo, *t.unc_lb);
    *open = cand;
}

// the row a picked node receives from its parent
HMPC_HD int32_t search_warm_index(int32_t wrow, int handdown) { return handdown ? wrow : -1; }

// ---- consume -------------------------------------------------------------------------------------------------------------------
#define SEARCH_PICK_STOP (-1)    // the tree has stopped (FAILED / OVERFLOW): this and its later picks are not consumed
#define SEARCH_PICK_LEAF 0       // pruned, infeasible or the new incumbent: the node stays a leaf
#define SEARCH_PICK_BRANCHED 1   // two children were appended at n - 2, n - 1: the caller writes their identifiers (search_child_fix)

// Node i of tree t was solved into row r of the pool; pos: branch_pos of its identifier.  Everything of the pick but the
// children's identifier rows.
HMPC_HD int search_consume_pick(const BranchDims &d, const SearchState &s, const SearchTree &t, int i, int32_t r, int pos, double tol)
{
    const int32_t status = s.p_status[r], iters = s.p_iters[r];
    if (status > HMPC_INFEASIBLE) {
        *t.state |= HMPC_SEARCH_FAILED;
        return SEARCH_PICK_STOP;
    }
    const double obj = s.p_obj[r];
    const int32_t word = branch_word(status, iters, obj, *t.ub - tol, pos, d.nfix);
    const int32_t n = *t.n;
    if ((word & HMPC_BRANCH_BRANCHED) && n + 2 > s.node_cap) { // (before anything of the pick is written)
        *t.state |= HMPC_SEARCH_OVERFLOW;
        return SEARCH_PICK_STOP;
    }
    ++*t.solves;
    if (iters & HMPC_ITERS_UNCERTIFIED) {
        ++*t.uncertified;
        *t.unc_lb = t.lb[i] < *t.unc_lb ? t.lb[i] : *t.unc_lb; // (the bound the node carried before its solve)
    }
    t.lb[i] = obj;
    t.row[i] = r;
    if (iters & HMPC_ITERS_WEAK) s.p_dual_obj[r] = -INFINITY;
    if (word & HMPC_BRANCH_COMPLETE) {
        *t.ub = obj;
        *t.inc = i;
        *t.inc_row = r;
    } else if (word & HMPC_BRANCH_BRANCHED) {
        for (int v = 0; v < 2; v++) {
            const int c = n + v;
            t.lb[c] = branch_child_lb(d, status, obj, s.p_dual + (size_t)r * d.n_dual, pos, v);
            t.row[c] = r;
            t.wrow[c] = branch_child_warm(word, r, 0);
            t.alive[c] = 1;
        }
        t.alive[i] = 0;
        *t.n = n + 2;
        return SEARCH_PICK_BRANCHED;
    }
    return SEARCH_PICK_LEAF;
}

// entry j of the v-branch's identifier, f the parent's entry
HMPC_HD int8_t search_child_fix(int8_t f, int j, int pos, int v) { return j == pos ? (int8_t)v : f; }

// ---- speculation: a launched pick rides with its descendants through its next binaries -----------------------------------------
// A block of L levels is the node and all its descendants through its next L free binaries, S(L) = 2^(L+1) - 1 rows in pre-order:
// row 0 the node, row 1 opens the 0-child's block of S(L-1) rows, row 1 + S(L-1) the 1-child's.  With hand-down off a record is a
// function of (x0, identifier) alone, so what rides along never changes a search, only the number of its launches; with hand-down
// on the descendants are solved cold (their parent rides in the same launch, as in tree_expand) and the equality is not bit for bit.
#define SEARCH_MAX_SPEC 4 // deepest speculation: blocks of at most S(4) = 31 rows

HMPC_HD int search_block_rows(int L) { return (2 << L) - 1; }

// levels of the block of a node whose identifier is fixed through pos: its free binaries bound the depth
HMPC_HD int search_block_levels(int spec, int nfix, int pos) { return spec < nfix - pos ? spec : nfix - pos; }

// the block of a pick: -1 where its record waits (the pick emits no row)
HMPC_HD int search_pick_levels(int32_t srow, int spec, int nfix, int pos) { return srow >= 0 ? -1 : search_block_levels(spec, nfix, pos); }
HMPC_HD int search_pick_rows(int lev) { return lev < 0 ? 0 : search_block_rows(lev); }

// Row q of a block of L levels: returns its depth m below the node; bit j < m of *bits is the value of binary pos + j on the path.
HMPC_HD int search_block_path(int L, int q, int *bits)
{
    int m = 0, b = 0;
    while (q > 0) { // row 0 of the block that is left is the node on the path; q - 1 counts into the 0-child's block, then the 1-child's
        L--;
        q--;
        const int half = search_block_rows(L);
        const int v = q >= half;
        q -= v ? half : 0;
        b |= v << m;
        m++;
    }
    *bits = b;
    return m;
}

// entry e of the identifier of such a row, f the node's entry
HMPC_HD int8_t search_block_fix(int8_t f, int e, int pos, int m, int bits) { return e >= pos && e < pos + m ? (int8_t)((bits >> (e - pos)) & 1) : f; }

// the v-child of a node consumed from row r with L levels below it: where its record waits, and how many levels lie below that
HMPC_HD int32_t search_child_srow(int32_t r, int L, int v) { return L > 0 ? r + 1 + v * search_block_rows(L - 1) : -1; }
HMPC_HD int32_t search_child_sleft(int L) { return L > 0 ? L - 1 : 0; }

// Where pick i's record is and how many levels wait below it: its waiting record, else the block staged for it (first: the
// block's first pool row, lev: its levels).
HMPC_HD bool search_waits(const SearchTree &t, int i) { return t.srow && t.srow[i] >= 0; }
HMPC_HD int32_t search_pick_row(const SearchTree &t, int i, int32_t first) { return search_waits(t, i) ? t.srow[i] : first; }
HMPC_HD int search_pick_left(const SearchTree &t, int i, int lev) { return search_waits(t, i) ? t.sleft[i] : lev; }

// search_consume_pick for a record with L levels of waiting descendants below it; a refused pick (FAILED, OVERFLOW) writes
// nothing, the waiting fields included.  The children's wrow stays the parent's row: it is used once a child without waiting
// descendants has children of its own to launch.
HMPC_HD int search_consume_waiting(const BranchDims &d, const SearchState &s, const SearchTree &t, int i, int32_t r, int L, int pos, double tol)
{
    const int32_t n = *t.n;
    const int act = search_consume_pick(d, s, t, i, r, pos, tol);
    if (act == SEARCH_PICK_STOP || !t.srow) return act;
    t.srow[i] = -1;
    if (act == SEARCH_PICK_BRANCHED)
        for (int v = 0; v < 2; v++) {
            t.srow[n + v] = search_child_srow(r, L, v);
            t.sleft[n + v] = search_child_sleft(L);
        }
    return act;
}

// a node that begins a step (begin, adopt) has no waiting record
HMPC_HD void search_clear_waiting(const SearchTree &t, int i)
{
    if (!t.srow) return;
    t.srow[i] = -1;
    t.sleft[i] = 0;
}

// ---- advance: the step that ended becomes the cover of the next one (hmpc_search_advance) --------------------------------------
// Per tree what tree_retain / fleet_stage_shift / tree_adopt_shifted of hmpc_tree.h do on the host, for slabs: which leaves a tree
// carries over, what the shift is given for each of them, and what the shift's outputs make of the tree.  The shift itself is
// hmpc_launch_shift (hmpc_shift.hip) between stage and adopt; its retain rule is search_retain_item.
struct SearchShift {
    int32_t *keep, *kept, *first;         // K x node_cap: a tree's kept nodes in list order; K: their number; K: its exclusive scan
    int32_t *word;                        // [0] kept leaves of all trees  [1] a tree is still running  [2] they fit the pool
    int32_t *owner, *src;                 // the staged leaves, tree by tree: tree, pool row its dual row is read from (row_cap: the zero row)
    int8_t *fix;                          // x nfix
    double *lb;
    double *u0, *e0, *x0_next;            // K x nu (zeros: the tree does not advance), K x nx, K x nx
    int8_t *fix_out;                      // what the shift returns for leaf b
    double *lb_out;
    uint8_t *flags;                       // bit 0: the shift kept it too, bit 1: reopened
    int32_t *cover, *reopened;            // K each
};

// a tree advances if and only if its search ended with an incumbent and nothing else -- proved (DONE) or cut off by its budget: the
// leaves of an unfinished tree still cover the binary cube, and every bound in it is still a dual bound
HMPC_HD bool search_advances(int32_t state)
{
    return state == (HMPC_SEARCH_DONE | HMPC_SEARCH_INCUMBENT) || state == (HMPC_SEARCH_BUDGET | HMPC_SEARCH_INCUMBENT);
}

// retain rule (tree_retain; both shift kernels): entry q < nub of an identifier against the incumbent's q-th binary of stage 0
HMPC_HD bool search_retain_item(int8_t f, double u) { return f < 0 || f == (int)rint(u); }

// u0: the incumbent's inputs of stage 0 (primal + o_u)
HMPC_HD bool search_retained(const BranchDims &d, const int8_t *fix, const double *u0)
{
    bool agree = true;
    for (int q = 0; q < d.nub && agree; q++) agree = search_retain_item(fix[q], u0[d.nu - d.nub + q]);
    return agree;
}

HMPC_HD const double *search_incumbent_u0(const BranchDims &d, const SearchState &s, const SearchTree &t)
{
    return s.p_primal + (size_t)*t.inc_row * d.n_primal + d.o_u;
}

// serial form of one tree's retain: its kept nodes in list order into keep (node_cap entries); returns their number
HMPC_HD int search_retain_serial(const BranchDims &d, const SearchState &s, const SearchTree &t, int32_t *keep)
{
    if (!search_advances(*t.state)) return 0;
    const double *u0 = search_incumbent_u0(d, s, t);
    int cnt = 0;
    for (int i = 0; i < *t.n; i++)
        if (t.alive[i] && search_retained(d, t.fix + (size_t)i * d.nfix, u0)) keep[cnt++] = i;
    return cnt;
}

// the pool row a staged leaf is shifted from: a node that carries none shifts from the zero row behind the pool
HMPC_HD int32_t search_shift_src(int32_t row, int32_t row_cap) { return row >= 0 ? row : row_cap; }

// everything of staged leaf b = node i of tree k but its identifier row
HMPC_HD void search_stage_leaf(const SearchState &s, const SearchTree &t, const SearchShift &g, int k, int i, size_t b)
{
    g.owner[b] = k;
    g.src[b] = search_shift_src(t.row[i], s.row_cap);
    g.lb[b] = t.lb[i];
}

// entry e of tree k's rows for the shift and for the next step: the applied input (zeros where the tree does not advance) and
// the next state (x1 + e0: ONE addition; a tree that does not advance keeps its state)
HMPC_HD double search_stage_u0(const double *primal_u0, bool advances, int e) { return advances ? primal_u0[e] : 0.0; }
HMPC_HD double search_stage_x0(const double *primal, int nx, bool advances, double x0, double e0, int e) { return advances ? primal[nx + e] + e0 : x0; }

// whether staged leaf b counts as reopened: the shift says so, or it carried no dual row
HMPC_HD bool search_leaf_reopened(const SearchState &s, const SearchShift &g, size_t b) { return (g.flags[b] & 2) != 0 || g.src[b] == s.row_cap; }

// staged leaf b becomes node j of its tree (everything but the identifier row); returns whether the shift kept it too
HMPC_HD bool search_adopt_leaf(const SearchTree &t, const SearchShift &g, int j, size_t b)
{
    t.lb[j] = g.lb_out[b];
    t.row[j] = (int32_t)b; // (a reopened leaf carries its row too: it is solved again before anything reads it)
    t.wrow[j] = -1;        // (the records of the step that ends here are not handed down across the shift)
    search_clear_waiting(t, j); // (nor do its waiting records survive it)
    t.alive[j] = 1;
    return (g.flags[b] & 1) != 0;
}

// the scalars of tree k as hmpc_search_begin_kernel leaves them; agreed: the shift kept every leaf the retain rule kept
HMPC_HD void search_adopt_scalars(const SearchState &s, const SearchTree &t, int k, int n, bool agreed)
{
    *t.n = n;
    *t.ub = INFINITY;
    *t.inc = -1;
    *t.inc_row = -1;
    *t.solves = 0;
    *t.uncertified = 0;
    *t.unc_lb = INFINITY;
    *t.state = agreed ? 0 : HMPC_SEARCH_FAILED;
    s.count[k] = 0;
    s.offset[k] = 0;
}

// ---- rebase: the trees of a step are carried to a neighbouring initial state of the SAME stage (hmpc_search_rebase) -------------
// x0 enters a node's QP only through the right-hand side of x_0 = x0, so every record's multipliers stay dual feasible and its dual
// (or Farkas) objective moves by -lam_0 . (x0_new - x0): the tail of both shift kernels (hmpc_shift.hip; controller.py:541-558),
// without the time shift.  retain -> offsets -> stage -> rebase-rows -> adopt share the staging of SearchShift with the advance:
// stage and adopt of a leaf ARE search_stage_leaf and search_adopt_leaf (flags bit 0 is always set here: nothing is dropped).

// a tree takes part if and only if it has neither failed nor outgrown its slab; a running tree does
HMPC_HD bool search_rebases(int32_t state) { return (state & (HMPC_SEARCH_FAILED | HMPC_SEARCH_OVERFLOW)) == 0; }

// retain rule: every alive node of a tree that takes part
HMPC_HD bool search_rebase_retained(uint8_t alive) { return alive != 0; }

// serial form of one tree's retain, as search_retain_serial
HMPC_HD int search_rebase_retain_serial(const SearchTree &t, int32_t *keep)
{
    if (!search_rebases(*t.state)) return 0;
    int cnt = 0;
    for (int i = 0; i < *t.n; i++)
        if (search_rebase_retained(t.alive[i])) keep[cnt++] = i;
    return cnt;
}

// The dual objective of a row at the new state: dual_obj - lam_0 . (x0_new - x0), clamped at 0 as the shift clamps it.  lam_0 is
// the row's first nx entries.  Serial, every product and every sum rounded on its own (no fma: the result is the same float64 on
// the host, on the device and in numpy).
// (The library is built with -ffp-contract=fast, under which the device back end fuses a product into a sum whatever a pragma says:
// on the device the product is made opaque before it is added -- an empty asm, no instruction.  The host builds with contraction off.)
#if defined(__HIP_DEVICE_COMPILE__)
#define SEARCH_ROUNDED(v) asm volatile("" : "+v"(v))
#else
#define SEARCH_ROUNDED(v) ((void)0)
#endif
HMPC_HD double search_rebase_obj(const double *dual, double dual_obj, const double *x0_new, const double *x0, int nx)
{
    double dot = 0.0;
    for (int j = 0; j < nx; j++) {
        const double delta = x0_new[j] - x0[j];
        double prod = dual[j] * delta;
        SEARCH_ROUNDED(prod);
        dot = dot + prod;
    }
    const double obj = dual_obj - dot;
    return obj > 0.0 ? obj : 0.0;
}

// the bound of a kept leaf from the bound it had and its row's new dual objective (the shift kernels' rule, their isinf test
// quoted); *flag: bit 0 kept, bit 1 reopened -- the flags of the shift
HMPC_HD double search_rebase_bound(double lb, double obj, uint8_t *flag)
{
    *flag = 1;
    double nlb;
    if (!isinf(lb)) nlb = obj;                       // a solved / bounded leaf: its bound is the moved dual objective
    else if (obj <= 0.0) { nlb = 0.0; *flag |= 2; } // the infeasibility proof did not survive: reopen
    else nlb = lb;                                   // still proved infeasible
    return nlb;
}

// a tree that does not take part becomes its root, as hmpc_search_begin without a cover leaves node 0 (its identifier row: all
// SEARCH_ROOT_FIX); returns the number of its nodes
#define SEARCH_ROOT_FIX ((int8_t)-1)
HMPC_HD int search_rebase_root(const SearchTree &t)
{
    t.lb[0] = -INFINITY;
    t.row[0] = -1;
    t.wrow[0] = -1;
    search_clear_waiting(t, 0);
    t.alive[0] = 1;
    return 1;
}

#endif // HMPC_SEARCH_CORE_H
