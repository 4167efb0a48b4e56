// hmpc_tree.h -- the host logic of the fleet driver (hmpc_fleet.hip), without anything of HIP in it.
//   per tree (tree_*): topology and bounds (identifiers, lower bounds, which pool row a node carries), candidate selection,
//     what rides in a launch (picked nodes, speculative descendants, predicted dives), prune / incumbent / branch on the
//     results, and the retain / adopt steps either side of the node shift;
//   per round and per step of the whole fleet (fleet_*), over plain pointers and the vector of trees: whether the pools may
//     start from zero, counting and staging a round's nodes, turning a round's results into the trees' waiting records,
//     the incumbents' rows, the outputs and the accounting that close a step, staging and adopting the leaves of a shift.
// hmpc_fleet.hip keeps what needs the device: buffers, copies, launches, synchronisation, timing, error messages.
// Semantics of the reference:
//   selection            warm_start_hmpc/branch_and_bound.py:462-470, 541-563 (best first, first wins ties)
//   prune / incumbent / branch   branch_and_bound.py:476-489; children in the order [0-branch, 1-branch], their bounds
//                        parent bound + multiplier of the tightened bound (controller.py:13-44, 395-429)
//   retain rule, shift   controller.py:431-564 (a leaf survives if its first-stage binaries agree with the applied input)
// Kept apart so that the very functions the library runs can be driven by CPU-computed QP results under AddressSanitizer /
// UBSan (tests/host/tree_driver.cpp, tests/test_sanitizers.py): the GPU pool has no device sanitizer.
#ifndef HMPC_TREE_H
#define HMPC_TREE_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/hmpc.h" // HMPC_OPTIMAL and the HMPC_ITERS_* flags of a record (by its place in the tree: this header needs no include path)

struct FleetResult { // a solved node waiting to be consumed by the search (speculative expansion)
    double obj, nu_lb, nu_ub; // objective; multipliers of the two bounds of the next binary in time
    int32_t row;              // its row in the pools
    bool vertex;              // optimal and polished: its record may be handed down to its children (hmpc_warm)
    bool failed;              // the solver did not converge on it (MAXITER / NUMERICAL): an error IF the search consumes it
    bool uncertified = false; // infeasible on the collapse of tau alone, no ray even loosely verified (HMPC_ITERS_UNCERTIFIED)
    bool digested = false;    // recorded from the device's digest (fleet_record_round_digest): the children's bounds were added there ...
    double child_lb[2] = {0.0, 0.0}; // ... obj + nu_ub (0-branch), obj + nu_lb (1-branch), the same float64 additions
};

struct FleetTree {
    std::vector<int8_t> fix;   // n x nfix, -1 free / 0 / 1 (chronological prefixes)
    std::vector<double> lb;    // lower bound, +inf: proved infeasible
    std::vector<int32_t> row;  // dual row of the current pool the node carries (own if solved, else parent's), -1: none
    std::vector<int32_t> wrow; // row of the parent's record (primal and dual pools of THIS step) to hand down, -1: none
    std::vector<uint8_t> alive;
    std::vector<int16_t> depth; // fixed binaries
    int n = 0;
    double ub = std::numeric_limits<double>::infinity();
    int inc = -1;               // incumbent node
    int32_t inc_row = -1;       // its row in the primal pool
    std::vector<double> primal; // its primal row
    int solves = 0;
    int uncertified = 0;        // nodes of this step pruned without a certificate ...
    double unc_lb = std::numeric_limits<double>::infinity(); // ... and the smallest bound such a node carried before its solve
    bool running = true;        // false once the MIQP of a step was infeasible (the loop has ended)
    std::vector<double> x0;     // state of the last solve
    std::unordered_map<std::string, FleetResult> cache; // key: the fixed prefix of the identifier
    std::unordered_map<int32_t, std::vector<int8_t>> rounded; // dive prediction: a solved vertex node's relaxed binaries, rounded, by pool row
};

inline void tree_reset_cold(FleetTree &t, int nfix)
{
    t.fix.assign(nfix, (int8_t)-1);
    t.lb.assign(1, -std::numeric_limits<double>::infinity());
    t.row.assign(1, -1);
    t.wrow.assign(1, -1);
    t.alive.assign(1, 1);
    t.depth.assign(1, 0);
    t.n = 1;
    t.running = true;
}

// a step begins: no incumbent, no results waiting
inline void tree_begin_step(FleetTree &t, const double *x0, int nx)
{
    t.ub = std::numeric_limits<double>::infinity();
    t.inc = -1;
    t.inc_row = -1;
    t.solves = 0;
    t.uncertified = 0;
    t.unc_lb = std::numeric_limits<double>::infinity();
    t.cache.clear();
    t.rounded.clear();
    t.x0.assign(x0, x0 + nx);
}

inline std::string tree_key(const int8_t *fx, int depth) { return std::string((const char *)fx, (size_t)depth); }

// candidates: alive, bound below the incumbent; the `width` smallest bounds, first wins ties
inline void tree_select(const FleetTree &t, int width, double tol, std::vector<int> &picks)
{
    picks.clear();
    if (!t.running) return;
    for (int i = 0; i < t.n; i++)
        if (t.alive[i] && t.lb[i] < t.ub - tol) picks.push_back(i);
    std::stable_sort(picks.begin(), picks.end(), [&](int a, int b) { return t.lb[a] < t.lb[b]; });
    if ((int)picks.size() > width) picks.resize(width);
}

// What has to be launched for picked node i: the node itself unless its result is waiting, its descendants through the next
// `speculation` binaries, and -- dive prediction -- the rest of the dive its parent's rounded relaxed binaries predict, with
// the sibling of every step.  emit(identifier row, depth, row of the record to hand down or -1) is called once per node.
template <class Emit>
inline void tree_expand(const FleetTree &t, int i, int nfix, int speculation, bool dive, bool handdown, std::vector<int8_t> &level,
                        std::vector<int8_t> &next, Emit emit)
{
    const int8_t *fx = t.fix.data() + (size_t)i * nfix;
    if (t.cache.count(tree_key(fx, t.depth[i]))) return;
    level.assign(fx, fx + nfix);
    int depth = t.depth[i];
    for (int s = 0; s <= speculation; s++) {
        const size_t cnt = level.size() / nfix;
        next.clear();
        for (size_t q = 0; q < cnt; q++) {
            const int8_t *row = level.data() + q * nfix;
            // hand-down: the picked node receives its parent's record (solved in an earlier round of this step); a
            // speculative descendant's parent rides in this very launch
            if (s == 0 || !t.cache.count(tree_key(row, depth))) emit(row, depth, (s == 0 && handdown) ? t.wrow[i] : -1);
            if (s < speculation && depth < nfix)
                for (int v = 0; v < 2; v++) {
                    next.insert(next.end(), row, row + nfix);
                    next[next.size() - nfix + depth] = (int8_t)v;
                }
        }
        if (next.empty()) break;
        level.swap(next);
        depth++;
    }
    if (dive && t.wrow[i] >= 0) {
        auto pr = t.rounded.find(t.wrow[i]);
        if (pr != t.rounded.end()) {
            level.assign(fx, fx + nfix); // the predicted path, one binary more per step
            for (int j = t.depth[i]; j < nfix; j++) {
                for (int side = 0; side < 2; side++) { // the sibling of the step, then the step itself
                    level[j] = side == 0 ? (int8_t)(1 - pr->second[j]) : pr->second[j];
                    if (t.cache.count(tree_key(level.data(), j + 1))) continue;
                    emit(level.data(), j + 1, -1); // (its parent rides in this very launch)
                }
            }
        }
    }
}

// prune / incumbent / branch, node by node in selection order (branch_and_bound.py:476-489).
// Returns 0, or 1: a selected node has no result, 2: the solver did not converge on a node the search consumes.
inline int tree_consume(FleetTree &t, const std::vector<int> &picks, int nfix, double tol)
{
    for (int i : picks) {
        auto it = t.cache.find(tree_key(t.fix.data() + (size_t)i * nfix, t.depth[i]));
        if (it == t.cache.end()) return 1;
        const FleetResult e = it->second;
        t.cache.erase(it);
        // (a speculative descendant that did not converge is an error only here, when the search gets to it: the result of a
        // step does not depend on what rode along)
        if (e.failed) return 2;
        const double obj = e.obj;
        t.solves++;
        if (e.uncertified) { // (pruned on the collapse of tau alone: counted, and reported if the step's optimum rests on it)
            t.uncertified++;
            t.unc_lb = std::min(t.unc_lb, t.lb[i]);
        }
        t.lb[i] = obj;
        t.row[i] = e.row;
        const double cutoff = t.ub - tol;
        if (obj >= cutoff) continue;
        const int d = t.depth[i];
        if (d == nfix) { // every binary fixed: new incumbent
            t.ub = obj;
            t.inc = i;
            t.inc_row = e.row; // (its primal row is fetched once, at the end of the step, with the others')
        } else { // branch on the next binary in time; child bound = parent bound + multiplier of the tightened bound
            for (int v = 0; v < 2; v++) {
                const size_t c = t.n;
                t.fix.resize((c + 1) * nfix);
                std::memcpy(t.fix.data() + c * nfix, t.fix.data() + (size_t)i * nfix, nfix);
                t.fix[c * nfix + d] = (int8_t)v;
                t.lb.push_back(e.digested ? e.child_lb[v] : obj + (v == 1 ? e.nu_lb : e.nu_ub));
                t.row.push_back(e.row);
                t.wrow.push_back(e.vertex ? e.row : -1);
                t.alive.push_back(1);
                t.depth.push_back((int16_t)(d + 1));
                t.n++;
            }
            t.alive[i] = 0;
        }
    }
    return 0;
}

inline int tree_leaves(const FleetTree &t)
{
    int c = 0;
    for (int i = 0; i < t.n; i++) c += t.alive[i];
    return c;
}

// Retain rule of the node shift (controller.py:431-501): the leaves whose first-stage binaries agree with the applied
// binaries u_b (rounded).  u: the incumbent's inputs of stage 0 (nu entries).
inline void tree_retain(const FleetTree &t, const double *u, int nuc, int nub, int nfix, std::vector<int> &keep)
{
    keep.clear();
    for (int i = 0; i < t.n; i++) {
        if (!t.alive[i]) continue;
        bool agree = true;
        for (int q = 0; q < nub && agree; q++) {
            const int fq = t.fix[(size_t)i * nfix + q];
            agree = fq < 0 || fq == (int)std::rint(u[nuc + q]);
        }
        if (agree) keep.push_back(i);
    }
}

// The shifted leaves become the next tree: identifiers move one stage towards the present; leaf j of `keep` carries pool
// row row0 + j, the bound lb[j]; flags[j] bit 1: the shift reopened it.  Returns the number of reopened leaves.
inline int tree_adopt_shifted(FleetTree &t, const std::vector<int> &keep, const double *lb, const uint8_t *flags, int32_t row0, int nub, int nfix)
{
    const size_t n = keep.size();
    std::vector<int8_t> nfixv(n * nfix, (int8_t)-1);
    std::vector<double> nlb(n);
    std::vector<int32_t> row(n);
    std::vector<int16_t> depth(n);
    int reop = 0;
    for (size_t j = 0; j < n; j++) {
        const int i = keep[j];
        std::memcpy(nfixv.data() + j * nfix, t.fix.data() + (size_t)i * nfix + nub, nfix - nub);
        nlb[j] = lb[j];
        reop += (flags[j] & 2) != 0;
        row[j] = row0 + (int32_t)j; // (a reopened leaf carries its row too: it is re-solved before anything reads it)
        depth[j] = (int16_t)std::max(0, (int)t.depth[i] - nub);
    }
    t.fix.swap(nfixv);
    t.lb.swap(nlb);
    t.row.swap(row);
    t.wrow.assign(n, -1); // (the records of the step that ends here are not handed down across the shift)
    t.depth.swap(depth);
    t.alive.assign(n, 1);
    t.n = (int)n;
    return reop;
}

// ---- the fleet: what a round and a step do with all trees at once ----

struct FleetDims { // sizes of a problem as the fleet's host logic needs them
    int nx, nu, nub, nuc, T, nfix; // nfix = T nub: length of a node's identifier
    int n_primal, n_dual;          // lengths of a record's primal and dual row (hmpc_record_sizes)
    int o_lb;                      // offset in the dual row of the multipliers of the binaries' bounds: nu_lb, then nu_ub (nfix each)
};

inline FleetDims fleet_dims(int nx, int nu, int nub, int T, int nc, int ncL, int nq, int nr, int nqT)
{
    const int o_lb = (T + 1) * nx + (T - 1) * nc + ncL;
    return FleetDims{nx, nu, nub, nu - nub, T, T * nub, (T + 1) * nx + T * nu, o_lb + 2 * T * nub + T * nq + nqT + T * nr, o_lb};
}

struct FleetExpansion { // what rides in a round besides the picked nodes (tree_expand), and the scratch of the expansion
    int speculation;
    bool dive, handdown;
    std::vector<int8_t> level, next; // identifiers of one level of a speculative expansion
};

struct FleetLaunch { int k, depth; }; // a node of a round: its loop and the number of its fixed binaries

// Rows nobody references can be reclaimed: when every tree is cold (no node carries a row of its own or of its parent) the
// pools may start from zero again.  Without this a fleet that is reset and solved at every step, never shifted -- the cold
// searches of fleet.closed_loop_study -- kept every row ever written: 880 k rows of ~8 KB over the published sd = .01
// study, 25-30 GB with the spare pool and the regrow copies (only the shift compacts).
inline bool fleet_pools_idle(const std::vector<FleetTree> &trees)
{
    for (const FleetTree &t : trees)
        for (int i = 0; i < t.n; i++)
            if (t.row[i] >= 0 || t.wrow[i] >= 0) return false;
    return true;
}

// What a round launches: for every picked node of every tree what tree_expand emits, loop by loop in selection order.
// emit(loop, identifier row, depth, row of the record to hand down or -1).
template <class Emit>
inline void fleet_walk_round(const std::vector<FleetTree> &trees, const std::vector<std::vector<int>> &picks, int nfix, FleetExpansion &ex, Emit emit)
{
    for (size_t k = 0; k < trees.size(); k++)
        for (int i : picks[k])
            tree_expand(trees[k], i, nfix, ex.speculation, ex.dive, ex.handdown, ex.level, ex.next,
                        [&](const int8_t *row, int depth, int32_t widx) { emit((int)k, row, depth, widx); });
}

// Number of nodes of the round: what the staging buffers must hold before fleet_fill_round writes them.
inline size_t fleet_count_round(const std::vector<FleetTree> &trees, const std::vector<std::vector<int>> &picks, const FleetDims &d, FleetExpansion &ex)
{
    size_t B = 0;
    fleet_walk_round(trees, picks, d.nfix, ex, [&](int, const int8_t *, int, int32_t) { B++; });
    return B;
}

// Stages the round: identifiers into fix (B x nfix), initial states into x0 (B x nx), the rows to hand down into widx (B),
// loop and depth of every node into launch.  Returns 1 if a node receives a record (some widx >= 0), 0 if none does, and
// -1 if the walk emitted a number of nodes other than B (nothing is written past node B).
inline int fleet_fill_round(const std::vector<FleetTree> &trees, const std::vector<std::vector<int>> &picks, const FleetDims &d, FleetExpansion &ex, size_t B,
                            int8_t *fix, double *x0, int32_t *widx, std::vector<FleetLaunch> &launch)
{
    size_t b = 0;
    bool any_warm = false;
    launch.clear();
    fleet_walk_round(trees, picks, d.nfix, ex, [&](int k, const int8_t *row, int depth, int32_t w) {
        if (b < B) {
            std::memcpy(fix + b * d.nfix, row, d.nfix);
            std::memcpy(x0 + b * d.nx, trees[k].x0.data(), d.nx * sizeof(double));
            widx[b] = w;
            any_warm |= w >= 0;
            launch.push_back({k, depth});
        }
        b++;
    });
    return b != B ? -1 : any_warm;
}

// The results of a round become records waiting in their trees' caches.  Node q of the round: identifier fix[q], pool row
// row0 + q, objective obj[q], status[q], iters[q] with the HMPC_ITERS_* flags; nu + q * nu_stride: the multipliers of the
// binaries' bounds (nu_lb then nu_ub, nfix each); primal + q * primal_stride: its primal row -- null without dive
// prediction, else the rounded relaxed binaries of every vertex node are kept for its descendants' dives.
// Returns the number of nodes whose handed-down active set verified; appends to `weak` the nodes that are infeasible without
// a ray that proves it to tolerance (HMPC_ITERS_WEAK): they prune at this step only, so their dual objective has to become
// -inf, with which the shift reopens the leaf whatever the model error (controller.py:555-558).
inline int fleet_record_round(std::vector<FleetTree> &trees, const std::vector<FleetLaunch> &launch, const FleetDims &d, int32_t row0, size_t B,
                              const int8_t *fix, const double *obj, const int32_t *status, const int32_t *iters, const double *nu, size_t nu_stride,
                              const double *primal, size_t primal_stride, std::vector<int32_t> &weak)
{
    int handed = 0;
    for (size_t q = 0; q < B; q++) {
        if (iters[q] & HMPC_ITERS_WEAK) weak.push_back((int32_t)q);
        handed += (iters[q] & HMPC_ITERS_HANDED) != 0;
        const int dep = launch[q].depth;
        const double *nu_ = nu + q * nu_stride;
        FleetTree &t = trees[launch[q].k];
        FleetResult e{obj[q], dep < d.nfix ? nu_[dep] : 0.0, dep < d.nfix ? nu_[d.nfix + dep] : 0.0, row0 + (int32_t)q,
                      status[q] == HMPC_OPTIMAL && (iters[q] & HMPC_ITERS_POLISHED) != 0, status[q] > 1, (iters[q] & HMPC_ITERS_UNCERTIFIED) != 0};
        if (primal && e.vertex && dep < d.nfix) {
            std::vector<int8_t> bits(d.nfix);
            const double *u = primal + q * primal_stride + (size_t)(d.T + 1) * d.nx;
            for (int j = 0; j < d.nfix; j++) bits[j] = u[(j / d.nub) * d.nu + d.nuc + (j % d.nub)] > 0.5 ? 1 : 0;
            t.rounded.emplace(e.row, std::move(bits));
        }
        t.cache.emplace(tree_key(fix + q * d.nfix, dep), e);
    }
    return handed;
}

// The same from the device's digest of the round (hmpc_branch.hip, the definitions of hmpc_branch.h) instead of the records:
// node q's objective obj[q], word[q] (HMPC_BRANCH_* of include/hmpc.h: what status and the flags of iters said), pos[q] (the
// number of its fixed binaries: the identifiers of a fleet are chronological prefixes), lb2 + 2 q: the bounds of its two children
// (0-branch first), bits + q * words: its rounded relaxed binaries, one bit each -- null without dive prediction.  No list
// of weak nodes: the digest kernel has written their dual objectives.  Returns the number of nodes whose handed-down active set
// verified, or -1 if the device's pos of a node is not the depth the host launched it with (nothing is recorded from there on).
inline int fleet_record_round_digest(std::vector<FleetTree> &trees, const std::vector<FleetLaunch> &launch, const FleetDims &d, int32_t row0, size_t B,
                                     const int8_t *fix, const double *obj, const int32_t *word, const int32_t *pos, const double *lb2,
                                     const uint64_t *bits, size_t words)
{
    int handed = 0;
    for (size_t q = 0; q < B; q++) {
        const int dep = launch[q].depth;
        if (pos[q] != dep) return -1;
        handed += (word[q] & HMPC_BRANCH_HANDED) != 0;
        FleetTree &t = trees[launch[q].k];
        FleetResult e{obj[q], 0.0, 0.0, row0 + (int32_t)q, (word[q] & HMPC_BRANCH_VERTEX) != 0, (word[q] & HMPC_BRANCH_FAILED) != 0,
                      (word[q] & HMPC_BRANCH_UNCERTIFIED) != 0, true, {lb2[2 * q], lb2[2 * q + 1]}};
        if (bits && e.vertex && dep < d.nfix) {
            std::vector<int8_t> rounded(d.nfix);
            for (int j = 0; j < d.nfix; j++) rounded[j] = (int8_t)((bits[q * words + j / 64] >> (j % 64)) & 1);
            t.rounded.emplace(e.row, std::move(rounded));
        }
        t.cache.emplace(tree_key(fix + q * d.nfix, dep), e);
    }
    return handed;
}

// rows[k]: the primal-pool row of loop k's incumbent, -1 for a loop that has none.  Returns whether any loop has one.
inline bool fleet_incumbent_rows(const std::vector<FleetTree> &trees, int32_t *rows)
{
    bool any = false;
    for (size_t k = 0; k < trees.size(); k++) {
        rows[k] = (trees[k].running && trees[k].inc >= 0) ? trees[k].inc_row : -1;
        any |= rows[k] >= 0;
    }
    return any;
}

struct FleetUncertified { // prunes without a certificate (HMPC_ITERS_UNCERTIFIED) of one step
    long long pruned = 0;  // such nodes
    long long resting = 0; // searches whose optimum rests on one: its bound lay below the final incumbent
    double unc_lb = 0, ub = 0; // that bound and that incumbent of the first such search
};

// A step ends.  prow: K primal rows, row k that of loop k's incumbent where rows[k] >= 0 (fleet_incumbent_rows; may be null
// if no loop has one).  Every tree takes its incumbent's row; the outputs (each may be null) are written, NaN in u0 / x1 for
// a loop without incumbent; such a loop's MIQP was infeasible and the loop ends here (statistical_analysis.py:99-108);
// the records nobody consumed are dropped.
inline FleetUncertified fleet_close_step(std::vector<FleetTree> &trees, const FleetDims &d, const int32_t *rows, const double *prow, double *cost, double *u0,
                                         double *x1, int32_t *solves, int32_t *n_leaves)
{
    FleetUncertified unc;
    for (size_t k = 0; k < trees.size(); k++) {
        FleetTree &t = trees[k];
        if (rows[k] >= 0) t.primal.assign(prow + k * d.n_primal, prow + (k + 1) * d.n_primal);
        if (t.uncertified) {
            unc.pruned += t.uncertified;
            if (t.unc_lb < t.ub) {
                if (!unc.resting) { unc.unc_lb = t.unc_lb; unc.ub = t.ub; }
                unc.resting++;
            }
            t.uncertified = 0;
        }
        t.cache.clear();
        if (cost) cost[k] = t.running ? t.ub : std::numeric_limits<double>::infinity();
        if (solves) solves[k] = t.solves;
        if (n_leaves) n_leaves[k] = t.running ? tree_leaves(t) : 0;
        const bool ok = t.running && t.inc >= 0;
        for (int j = 0; j < d.nu && u0; j++) u0[k * d.nu + j] = ok ? t.primal[(size_t)(d.T + 1) * d.nx + j] : NAN;
        for (int j = 0; j < d.nx && x1; j++) x1[k * d.nx + j] = ok ? t.primal[d.nx + j] : NAN;
        if (t.running && t.inc < 0) t.running = false;
    }
    return unc;
}

// The leaves every running loop with an incumbent keeps across the shift (tree_retain); cover and reopened (each may be
// null) start at zero.  Returns their number over all loops.
inline size_t fleet_retain_leaves(const std::vector<FleetTree> &trees, const FleetDims &d, std::vector<std::vector<int>> &keep, int32_t *cover, int32_t *reopened)
{
    size_t B = 0;
    for (size_t k = 0; k < trees.size(); k++) {
        const FleetTree &t = trees[k];
        keep[k].clear();
        if (cover) cover[k] = 0;
        if (reopened) reopened[k] = 0;
        if (!t.running || t.inc < 0) continue;
        tree_retain(t, t.primal.data() + (size_t)(d.T + 1) * d.nx, d.nuc, d.nub, d.nfix, keep[k]);
        B += keep[k].size();
    }
    return B;
}

// Stages the shift: per loop the state of the last solve (hx, K x nx), the applied input (hu, K x nu; zero for a loop that
// keeps nothing) and the model error (he <- e0, K x nx); per kept leaf its identifier, loop, pool row and bound.
// Returns false if a leaf carries no multipliers.
inline bool fleet_stage_shift(const std::vector<FleetTree> &trees, const FleetDims &d, const std::vector<std::vector<int>> &keep, const double *e0, double *hx,
                              double *hu, double *he, int8_t *fix, int32_t *owner, int32_t *src, double *lb)
{
    size_t b = 0;
    for (size_t k = 0; k < trees.size(); k++) {
        const FleetTree &t = trees[k];
        std::memcpy(hx + k * d.nx, t.x0.data(), d.nx * sizeof(double));
        std::memcpy(he + k * d.nx, e0 + k * d.nx, d.nx * sizeof(double));
        for (int j = 0; j < d.nu; j++) hu[k * d.nu + j] = keep[k].empty() ? 0.0 : t.primal[(size_t)(d.T + 1) * d.nx + j];
        for (int i : keep[k]) {
            if (t.row[i] < 0) return false;
            std::memcpy(fix + b * d.nfix, t.fix.data() + (size_t)i * d.nfix, d.nfix);
            owner[b] = (int32_t)k;
            src[b] = t.row[i];
            lb[b] = t.lb[i];
            b++;
        }
    }
    return true;
}

// The shifted leaves are the next trees (tree_adopt_shifted): leaf b of the staging order carries row b of the next pool,
// the bound lb[b] and flags[b] -- bit 0: the device kept it too, bit 1: the shift reopened it.  cover[k] / reopened[k] (each
// may be null): leaves loop k carries over, and how many of them reopened.  Returns false if the device dropped a leaf the
// host kept: the two disagree on the retain rule.
inline bool fleet_adopt_shift(std::vector<FleetTree> &trees, const FleetDims &d, const std::vector<std::vector<int>> &keep, const double *lb, const uint8_t *flags,
                              int32_t *cover, int32_t *reopened)
{
    size_t b = 0;
    for (size_t k = 0; k < trees.size(); k++) {
        const size_t n = keep[k].size();
        if (n == 0) continue;
        for (size_t j = 0; j < n; j++)
            if (!(flags[b + j] & 1)) return false;
        const int reop = tree_adopt_shifted(trees[k], keep[k], lb + b, flags + b, (int32_t)b, d.nub, d.nfix);
        b += n;
        if (cover) cover[k] = (int32_t)n;
        if (reopened) reopened[k] = reop;
    }
    return true;
}

#endif // HMPC_TREE_H
