/*
 * hmpc_search_anytime.h -- device searches under a deadline: node rules, solve budgets, proven bounds.
 *
 * include/hmpc_search.h searches best-first until the optimum is proven.  A real-time caller needs three things more, all behind
 * the entries of this header; a search that never calls them behaves as hmpc_search.h says, bit for bit.
 *
 * Rule (hmpc_search_set_rule): the order in which a round picks among a tree's candidates.  The candidates are unchanged
 * (alive && lb < ub - tol), and a round still picks the `width` first of them in the rule's order -- the reference's
 * candidate_selection applied repeatedly (warm_start_hmpc/branch_and_bound.py:501-561).  Slabs are in list order and children are
 * appended, so
 *   HMPC_RULE_BEST_FIRST      the smallest (lb, index): the rule of hmpc_search.h
 *   HMPC_RULE_DEPTH_FIRST     the LARGEST index (the reference pops the last candidate of its list)
 *   HMPC_RULE_BREADTH_FIRST   the SMALLEST index
 *   HMPC_RULE_DIVE_THEN_BEST  per tree, decided at select: depth-first while the tree has no incumbent (inc < 0), best-first from then on
 * A rule changes nothing else: consume is serial within a tree, and speculation keeps its invariant under every rule.
 *
 * Budget (hmpc_search_set_budget): a tree consumes at most max_solves picks per step (`solves` of hmpc_search_results counts them;
 * begin, advance and rebase reset it).  At select a running tree picks min(width, max_solves - solves) candidates.  A running tree
 * that has candidates and no budget left gets the state HMPC_SEARCH_BUDGET | (inc >= 0 ? HMPC_SEARCH_INCUMBENT : 0), written where
 * HMPC_SEARCH_DONE is written (a round refused with HMPC_ETOOBIG changes nothing, these words included); a tree without candidates
 * gets DONE as ever, whatever its budget.  hmpc_search_run ends, as ever, when a select stages no pick.
 *
 * Bounds (hmpc_search_bounds): what a search proves as it stands, per tree:
 *   lower = min(min over alive nodes of lb, unc_lb) -- the leaves cover the binary cube and every lb is a dual bound, so this is a
 *           lower bound of the MIQP's optimal cost; a leaf pruned on an uncertified record counts for the bound it carried before
 *           (unc_lb).  +inf for a tree without alive nodes, -inf for a root.  Never NaN: a NaN bound is skipped.
 *   upper = ub (+inf without incumbent)
 *   open  = the number of candidates at `tol`
 *
 * Advance: hmpc_search_advance additionally accepts a tree whose state is exactly HMPC_SEARCH_BUDGET | HMPC_SEARCH_INCUMBENT.  The
 * leaves of an unfinished tree still cover the binary cube and their bounds are still dual bounds, so retain -> shift -> adopt are
 * valid as they stand; the incumbent's u0 is the input applied.  A budget-stopped tree without an incumbent gets an empty cover, as
 * any tree without one.  hmpc_search_rebase takes such trees as it takes running ones.
 *
 * The deadline recipe: set_budget(m) -> run -> results + bounds -> advance; in idle time, optionally, set_budget(-1) -> run first.
 */
#ifndef HMPC_SEARCH_ANYTIME_H
#define HMPC_SEARCH_ANYTIME_H

#include "hmpc_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HMPC_RULE_BEST_FIRST     0   /* today's rule; a new search has it */
#define HMPC_RULE_DEPTH_FIRST    1   /* LIFO: the candidate with the LARGEST index */
#define HMPC_RULE_BREADTH_FIRST  2   /* FIFO: the candidate with the SMALLEST index */
#define HMPC_RULE_DIVE_THEN_BEST 3   /* per tree: depth-first while it has no incumbent (inc < 0 at select), best-first from then on */
#define HMPC_SEARCH_BUDGET 0x10      /* state word: stopped by its solve budget with candidates left */

/* The rule of the rounds to come; it holds until it is changed, across begin, advance and rebase.
 * HMPC_EINVAL without touching the GPU: a rule outside 0 .. 3 (checked first), a null search, a staged round. */
int hmpc_search_set_rule(hmpc_search *s, int32_t rule);

/* The budget of every tree, max_solves < 0: none (the default).  Every tree whose state is exactly BUDGET or BUDGET | INCUMBENT
 * runs again (state 0): the next select stops it once more if the new budget is exhausted too -- this is how a cut-off search is
 * continued in idle time.  Asynchronous on `stream`.  HMPC_EINVAL: a null search, a staged round. */
int hmpc_search_set_budget(hmpc_search *s, int32_t max_solves, void *stream);

/* lower, upper, open: host arrays of K each, any may be NULL.  One synchronisation.
 * HMPC_EINVAL: a null search, no step has begun, a staged round. */
int hmpc_search_bounds(hmpc_search *s, double tol, double *lower, double *upper, int32_t *open, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HMPC_SEARCH_ANYTIME_H */
