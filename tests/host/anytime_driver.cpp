// anytime_driver.cpp -- the CPU form of the rounds of hmpc_search under a rule and a solve budget (include/hmpc_search_anytime.h):
// speculation_driver.cpp's serial walk over K trees with the per-tree functions of csrc/hmpc_search.h, selecting with
// search_select_anytime, stopping with search_stop_word, re-opening with search_budget_stopped and bounding with search_bounds_serial --
// what the kernels of csrc/hmpc_search.hip run per workgroup, wavefront or thread --, built with -fsanitize=address,undefined by
// tests/test_search_anytime_host.py.  It restates none of the arithmetic.  Every array is exactly as long as the sizes say -- the pool
// has row_cap rows, a tree's picks SEARCH_MAX_WIDTH entries --, so an index beyond one is a sanitizer report.
// defect (for the tests' planted defects, around the header's functions, never in them):
//   1  depth-first orders by the LARGEST BOUND (the key handed to search_take is -lb) instead of the largest index
//   2  the budget caps a round at min(width, max_solves) without looking at solves (the tree's counter is hidden from the selection)
//   3  lower forgets unc_lb (the tree's unc_lb is hidden from search_bounds_serial)
//
//   anytime_driver <in> <out>
//   in : int32 nx nu nub T nc ncT nq nr nqT K node_cap width handdown defect has_cover rounds depth row_cap rule max_solves | float64 tol
//        | if has_cover: int32 count[K], then per tree int8 fix (count x T nub), float64 lb[count]
//        | per round: int32 set (1: hmpc_search_set_budget(budget) comes before the round), budget, B
//          | float64 obj[B] dual_obj[B] | int32 status[B] iters[B] | float64 primal (B x n_primal) dual (B x n_dual)
//   out: int32 rounds walked, refused (the next round did not fit row_cap: nothing of it was done)
//        | per round: int32 B, P, tree[B], node[B], warm[B] | int8 fix (B x T nub)
//          | after the round (consumed if P > 0): int32 state[K] | float64 lower[K] upper[K] | int32 open[K]
//        | per tree: int32 n inc inc_row solves uncertified state | float64 ub unc_lb | int8 fix (n x T nub) | float64 lb[n]
//          | int32 row[n] wrow[n] | uint8 alive[n] | int32 srow[n] sleft[n]
//        | int32 rows | float64 dual_obj[rows] of the pool
// A round without a pick is walked too (nothing is consumed): a later set_budget may let its trees run again.
// A round that stages another number of rows than it has records for ends the walk with exit code 3.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hmpc_search.h"

template <class T> static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "anytime_driver: input too short\n");
        exit(2);
    }
    return v;
}

template <class T> static void put(FILE *f, const T *p, size_t n)
{
    if (n && fwrite(p, sizeof(T), n, f) != n) exit(2);
}

struct Round {
    int32_t set, budget, B;
    std::vector<double> obj, dual_obj, primal, dual;
    std::vector<int32_t> status, iters;
};

// defect 1: search_select_anytime's loop with the key -lb where the tree's rule is depth-first
static int select_depth_by_bound(const SearchTree &t, int limit, double tol, int32_t *picks)
{
    double pk = -INFINITY;
    int pi = -1, cnt = 0;
    while (cnt < limit) {
        double bk = 0.0;
        int bi = -1;
        for (int i = 0; i < *t.n; i++)
            if (search_candidate(t.alive[i], t.lb[i], *t.ub, tol) && search_take(bk, bi, -t.lb[i], i, pk, pi)) { bk = -t.lb[i]; bi = i; }
        if (bi < 0) break;
        picks[cnt++] = bi;
        pk = bk;
        pi = bi;
    }
    return cnt;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> n = take<int32_t>(f, 20);
    const BranchDims d = branch_dims(n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8]);
    const int K = n[9], node_cap = n[10], width = n[11], handdown = n[12], defect = n[13], spec = n[16], row_cap = n[17], rule = n[18];
    const double tol = take<double>(f, 1)[0];
    const size_t nfix = (size_t)d.nfix, nodes = (size_t)K * node_cap, rows = (size_t)row_cap;
    if (width < 1 || width > SEARCH_MAX_WIDTH || spec < 0 || spec > SEARCH_MAX_SPEC || row_cap < 0 || rule < 0 || rule > HMPC_RULE_DIVE_THEN_BEST) return 2;

    std::vector<int32_t> count(K, 1);
    std::vector<std::vector<int8_t>> c_fix(K);
    std::vector<std::vector<double>> c_lb(K);
    if (n[14]) {
        count = take<int32_t>(f, K);
        for (int k = 0; k < K; k++) {
            if (count[k] < 0 || count[k] > node_cap) return 2;
            c_fix[k] = take<int8_t>(f, (size_t)count[k] * nfix);
            c_lb[k] = take<double>(f, count[k]);
        }
    }
    std::vector<Round> rounds(n[15]);
    for (Round &r : rounds) {
        const std::vector<int32_t> head = take<int32_t>(f, 3);
        r.set = head[0];
        r.budget = head[1];
        r.B = head[2];
        const size_t B = (size_t)r.B;
        r.obj = take<double>(f, B);
        r.dual_obj = take<double>(f, B);
        r.status = take<int32_t>(f, B);
        r.iters = take<int32_t>(f, B);
        r.primal = take<double>(f, B * d.n_primal);
        r.dual = take<double>(f, B * d.n_dual);
    }
    fclose(f);

    std::vector<int8_t> fix(nodes * nfix, 0);
    std::vector<double> lb(nodes, 0.0), ub(K), unc_lb(K), p_obj(rows), p_dobj(rows), p_primal(rows * d.n_primal), p_dual(rows * d.n_dual);
    std::vector<int32_t> row(nodes, 0), wrow(nodes, 0), srow(nodes, 5), sleft(nodes, 5), tn(K), inc(K), inc_row(K), solves(K), uncertified(K), state(K),
        p_status(rows), p_iters(rows), open(K, 0);
    std::vector<uint8_t> alive(nodes, 0);
    std::vector<int32_t> picks((size_t)K * SEARCH_MAX_WIDTH), plev((size_t)K * SEARCH_MAX_WIDTH), pfirst((size_t)K * SEARCH_MAX_WIDTH), cnt(K), offset(K), word(6);
    SearchState s{K, node_cap, row_cap, fix.data(), lb.data(), row.data(), wrow.data(), alive.data(), tn.data(), inc.data(), inc_row.data(), solves.data(),
                  uncertified.data(), state.data(), ub.data(), unc_lb.data(), nullptr, p_obj.data(), p_dobj.data(), p_status.data(), p_iters.data(),
                  p_primal.data(), p_dual.data(), picks.data(), cnt.data(), offset.data(), word.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                  srow.data(), sleft.data(), plev.data(), pfirst.data(), spec, rule, n[19] < 0 ? 0 : n[19] + 1, open.data()};

    for (int k = 0; k < K; k++) { // begin (no dual rows: the covers of this driver carry none)
        const SearchTree t = search_tree(s, d.nfix, k);
        for (int i = 0; i < count[k]; i++) {
            for (size_t e = 0; e < nfix; e++) t.fix[(size_t)i * nfix + e] = n[14] ? c_fix[k][(size_t)i * nfix + e] : (int8_t)-1;
            t.lb[i] = n[14] ? c_lb[k][i] : -INFINITY;
            t.row[i] = -1;
            t.wrow[i] = -1;
            search_clear_waiting(t, i);
            t.alive[i] = 1;
        }
        search_adopt_scalars(s, t, k, count[k], true);
    }
    int32_t row0 = 0;

    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    const long head = ftell(o);
    int32_t walked = 0, refused = 0;
    put(o, &walked, 1);
    put(o, &refused, 1);
    for (const Round &r : rounds) {
        if (r.set) { // hmpc_search_set_budget: the budget, then the trees it had stopped run again
            s.budget1 = r.budget < 0 ? 0 : r.budget + 1;
            for (int k = 0; k < K; k++)
                if (search_budget_stopped(state[k])) state[k] = 0;
        }
        // select: the picks, their blocks, the rows of every tree
        int32_t B = 0, P = 0;
        for (int k = 0; k < K; k++) {
            const SearchTree t = search_tree(s, d.nfix, k);
            const size_t p = (size_t)k * SEARCH_MAX_WIDTH;
            SearchTree u = t;
            int32_t none = 0;
            if (defect == 2) u.solves = &none;
            cnt[k] = search_select_anytime(u, s.rule, s.budget1, width, tol, picks.data() + p, &open[k]);
            if (defect == 1 && search_running(*t.state) && search_tree_rule(s.rule, *t.inc) == HMPC_RULE_DEPTH_FIRST)
                cnt[k] = select_depth_by_bound(t, cnt[k], tol, picks.data() + p);
            int32_t v = 0;
            for (int j = 0; j < cnt[k]; j++) {
                const int i = picks[p + j];
                plev[p + j] = search_pick_levels(t.srow[i], spec, d.nfix, branch_pos_serial(t.fix + (size_t)i * nfix, d.nfix));
                pfirst[p + j] = v;
                v += search_pick_rows(plev[p + j]);
            }
            offset[k] = B;
            B += v;
            P += cnt[k];
        }
        if ((long long)row0 + B > row_cap) { // the round is refused: nothing changes, the state words neither
            refused = 1;
            break;
        }
        if (B != r.B) {
            fprintf(stderr, "anytime_driver: round %d stages %d rows, the caller has records for %d\n", walked, B, r.B);
            return 3;
        }
        // stage
        std::vector<int32_t> b_tree(B, -7), b_node(B, -7), b_warm(B, -7);
        std::vector<int8_t> b_fix((size_t)B * nfix);
        for (int k = 0; k < K; k++) {
            if (cnt[k] == 0 && search_running(state[k])) state[k] = search_stop_word(inc[k], open[k]);
            for (int j = 0; j < cnt[k]; j++) {
                const size_t p = (size_t)k * SEARCH_MAX_WIDTH + j;
                const int i = picks[p];
                const int8_t *fx = fix.data() + ((size_t)k * node_cap + i) * nfix;
                const int pos = branch_pos_serial(fx, d.nfix);
                for (int q = 0; q < search_pick_rows(plev[p]); q++) {
                    const size_t b = (size_t)offset[k] + pfirst[p] + q;
                    int bits = 0;
                    const int m = search_block_path(plev[p], q, &bits);
                    for (size_t e = 0; e < nfix; e++) b_fix.at(b * nfix + e) = search_block_fix(fx[e], (int)e, pos, m, bits);
                    b_tree.at(b) = k;
                    b_node.at(b) = q == 0 ? i : -1;
                    b_warm.at(b) = q == 0 ? search_warm_index(wrow[(size_t)k * node_cap + i], handdown) : -1;
                }
            }
        }
        put(o, &B, 1);
        put(o, &P, 1);
        put(o, b_tree.data(), B);
        put(o, b_node.data(), B);
        put(o, b_warm.data(), B);
        put(o, b_fix.data(), b_fix.size());
        if (P > 0) {
            // the records take rows row0 .. row0 + B - 1
            for (int b = 0; b < B; b++) {
                const size_t q = (size_t)row0 + b;
                p_obj.at(q) = r.obj[b];
                p_dobj.at(q) = r.dual_obj[b];
                p_status.at(q) = r.status[b];
                p_iters.at(q) = r.iters[b];
                for (int e = 0; e < d.n_primal; e++) p_primal.at(q * d.n_primal + e) = r.primal[(size_t)b * d.n_primal + e];
                for (int e = 0; e < d.n_dual; e++) p_dual.at(q * d.n_dual + e) = r.dual[(size_t)b * d.n_dual + e];
            }
            // consume
            for (int k = 0; k < K; k++) {
                const SearchTree t = search_tree(s, d.nfix, k);
                for (int j = 0; j < cnt[k]; j++) {
                    const size_t p = (size_t)k * SEARCH_MAX_WIDTH + j;
                    const int i = picks[p];
                    const int8_t *fx = t.fix + (size_t)i * nfix;
                    const int pos = branch_pos_serial(fx, d.nfix);
                    const int c = *t.n;
                    const int32_t rr = search_pick_row(t, i, row0 + offset[k] + pfirst[p]);
                    const int L = search_pick_left(t, i, plev[p]);
                    const int act = search_consume_waiting(d, s, t, i, rr, L, pos, tol);
                    if (act == SEARCH_PICK_STOP) break;
                    if (act == SEARCH_PICK_BRANCHED)
                        for (int v = 0; v < 2; v++)
                            for (size_t e = 0; e < nfix; e++) fix.at(((size_t)k * node_cap + c + v) * nfix + e) = search_child_fix(fx[e], (int)e, pos, v);
                }
            }
            row0 += B;
        }
        // hmpc_search_bounds
        std::vector<double> lower(K), upper(K);
        std::vector<int32_t> cand(K);
        for (int k = 0; k < K; k++) {
            SearchTree u = search_tree(s, d.nfix, k);
            double none = INFINITY;
            if (defect == 3) u.unc_lb = &none;
            search_bounds_serial(u, tol, &lower[k], &cand[k]);
            upper[k] = ub[k];
        }
        put(o, state.data(), K);
        put(o, lower.data(), K);
        put(o, upper.data(), K);
        put(o, cand.data(), K);
        walked++;
    }
    for (int k = 0; k < K; k++) {
        const SearchTree t = search_tree(s, d.nfix, k);
        const int32_t sc[6] = {*t.n, *t.inc, *t.inc_row, *t.solves, *t.uncertified, *t.state};
        const double bd[2] = {*t.ub, *t.unc_lb};
        const size_t m = (size_t)*t.n;
        put(o, sc, 6);
        put(o, bd, 2);
        put(o, t.fix, m * nfix);
        put(o, t.lb, m);
        put(o, t.row, m);
        put(o, t.wrow, m);
        put(o, t.alive, m);
        put(o, t.srow, m);
        put(o, t.sleft, m);
    }
    put(o, &row0, 1);
    put(o, p_dobj.data(), (size_t)row0);
    fseek(o, head, SEEK_SET);
    put(o, &walked, 1);
    put(o, &refused, 1);
    fclose(o);
    return 0;
}
