// hmpc_search.h -- what one tree of a device-resident search does in a round (include/hmpc_search.h), item by item.
//
// Plain inline functions that compile for the device (hipcc) and for the host (g++), as hmpc_branch.h does: which nodes are
// candidates and in which order they are picked, and what consuming ONE pick does to its tree.  Every decision about a record
// is a function of hmpc_branch.h (branch_word, branch_child_lb, branch_child_warm; pos from branch_pos_*): nothing of it is
// restated here.  The kernels (hmpc_search.hip) supply the workgroup argmin, the scan over the trees and the lane loops over
// identifier rows; tests/host/search_driver.cpp walks the same functions serially under AddressSanitizer.
//
// Semantics: tree_select / tree_consume of hmpc_tree.h without speculation and dive (reference: branch_and_bound.py:462-489),
// with the record's decision taken as hmpc_branch_batch takes it (`obj < cutoff`: a NaN objective prunes).
#ifndef HMPC_SEARCH_CORE_H
#define HMPC_SEARCH_CORE_H

#include "../../include/hmpc_search.h"
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
    int32_t *word;                        // [0] B  [1] a tree has stopped FAILED / OVERFLOW  [2] a node receives a record  [3] the round fits the pool
    int8_t *b_fix;                        // the batch: B x nfix
    double *b_x0;                         // B x nx
    int32_t *b_warm, *b_tree, *b_node;    // B each
};

struct SearchTree { // one tree of it
    int8_t *fix;
    double *lb;
    int32_t *row, *wrow;
    uint8_t *alive;
    int32_t *n, *inc, *inc_row, *solves, *uncertified, *state;
    double *ub, *unc_lb;
};

HMPC_HD SearchTree search_tree(const SearchState &s, int nfix, int k)
{
    const size_t o = (size_t)k * s.node_cap;
    return SearchTree{s.fix + o * nfix, s.lb + o, s.row + o, s.wrow + o, s.alive + o, s.n + k, s.inc + k, s.inc_row + k, s.solves + k,
                      s.uncertified + k, s.state + k, s.ub + k, s.unc_lb + k};
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

#endif // HMPC_SEARCH_CORE_H
