// speculation_driver.cpp -- the CPU form of the rounds of hmpc_search at a speculation depth: search_driver.cpp's serial walk over K
// trees with the per-tree functions of csrc/hmpc_search.h, and with them the block arithmetic the kernels of csrc/hmpc_search.hip
// run per wavefront (search_pick_levels, search_block_path, search_block_fix, search_consume_waiting ...), built with
// -fsanitize=address,undefined by tests/test_search_speculation_host.py.  It restates none of the arithmetic.  Every array is exactly
// as long as the sizes say -- the pool has row_cap rows --, so an index beyond one is a sanitizer report.
// defect (for the tests' planted defects, around the header's functions, never in them):
//   1  the 1-child's waiting row is r + 2
//   2  waiting records survive begin
//
//   speculation_driver blocks <out> <depth> <fix entries ...>
//   out: int32 S | int8 identifiers (S x nfix) | int32 waiting rows of the children of every row (S x 2, block-relative) | int32 levels left at every row
//
//   speculation_driver walk <in> <out>
//   in : int32 nx nu nub T nc ncT nq nr nqT K node_cap width handdown defect has_cover rounds depth row_cap rebegin first_count | float64 tol
//        | if has_cover: int32 count[K], then per tree int8 fix (count x T nub), float64 lb[count]
//        | per round: int32 B | float64 obj[B] dual_obj[B] | int32 status[B] iters[B] | float64 primal (B x n_primal) dual (B x n_dual)
//        (rebegin: the round before which the step begins again from the covers, -1: never; first_count > 0: the FIRST begin takes
//        only that many leaves of every cover, so that the second one covers nodes the first step has appended)
//   out: int32 rounds walked, refused (the next round did not fit row_cap: nothing of it was done)
//        | per round: int32 B, P, tree[B], node[B], warm[B] | int8 fix (B x T nub)
//        | per tree: int32 n inc inc_row solves uncertified state | float64 ub unc_lb | int8 fix (n x T nub) | float64 lb[n]
//          | int32 row[n] wrow[n] | uint8 alive[n] | int32 srow[n] sleft[n]
//        | int32 rows | float64 dual_obj[rows] of the pool | int64 rounds, launches, rows launched, picks served from waiting records
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
        fprintf(stderr, "speculation_driver: input too short\n");
        exit(2);
    }
    return v;
}

template <class T> static void put(FILE *f, const T *p, size_t n)
{
    if (n && fwrite(p, sizeof(T), n, f) != n) exit(2);
}

static int blocks(int argc, char **argv)
{
    if (argc < 5) return 2;
    const int spec = atoi(argv[3]), nfix = argc - 4;
    std::vector<int8_t> fix(nfix);
    for (int e = 0; e < nfix; e++) fix[e] = (int8_t)atoi(argv[4 + e]);
    const int pos = branch_pos_serial(fix.data(), nfix), L = search_block_levels(spec, nfix, pos);
    const int32_t S = search_block_rows(L);
    std::vector<int8_t> ids((size_t)S * nfix);
    std::vector<int32_t> kids((size_t)S * 2, -1), left(S, -7);
    left[0] = L;
    for (int q = 0; q < S; q++) { // (pre-order: a row comes before its children)
        int bits = 0;
        const int m = search_block_path(L, q, &bits);
        for (int e = 0; e < nfix; e++) ids[(size_t)q * nfix + e] = search_block_fix(fix[e], e, pos, m, bits);
        for (int v = 0; v < 2; v++) {
            const int32_t c = kids.at((size_t)q * 2 + v) = search_child_srow(q, left.at(q), v);
            if (c >= 0) left.at(c) = search_child_sleft(left[q]);
        }
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    put(o, &S, 1);
    put(o, ids.data(), ids.size());
    put(o, kids.data(), kids.size());
    put(o, left.data(), left.size());
    fclose(o);
    return 0;
}

struct Round {
    int32_t B;
    std::vector<double> obj, dual_obj, primal, dual;
    std::vector<int32_t> status, iters;
};

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "blocks")) return blocks(argc, argv);
    if (argc != 4 || strcmp(argv[1], "walk")) return 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    const std::vector<int32_t> n = take<int32_t>(f, 20);
    const BranchDims d = branch_dims(n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8]);
    const int K = n[9], node_cap = n[10], width = n[11], handdown = n[12], defect = n[13], spec = n[16], row_cap = n[17], rebegin = n[18];
    const double tol = take<double>(f, 1)[0];
    const size_t nfix = (size_t)d.nfix, nodes = (size_t)K * node_cap, rows = (size_t)row_cap;
    if (width < 1 || width > SEARCH_MAX_WIDTH || spec < 0 || spec > SEARCH_MAX_SPEC || row_cap < 0) return 2;

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
        r.B = take<int32_t>(f, 1)[0];
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
        p_status(rows), p_iters(rows);
    std::vector<uint8_t> alive(nodes, 0);
    std::vector<int32_t> picks((size_t)K * SEARCH_MAX_WIDTH), plev((size_t)K * SEARCH_MAX_WIDTH), pfirst((size_t)K * SEARCH_MAX_WIDTH), cnt(K), offset(K), word(6);
    SearchState s{K, node_cap, row_cap, fix.data(), lb.data(), row.data(), wrow.data(), alive.data(), tn.data(), inc.data(), inc_row.data(), solves.data(),
                  uncertified.data(), state.data(), ub.data(), unc_lb.data(), nullptr, p_obj.data(), p_dobj.data(), p_status.data(), p_iters.data(),
                  p_primal.data(), p_dual.data(), picks.data(), cnt.data(), offset.data(), word.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                  srow.data(), sleft.data(), plev.data(), pfirst.data(), spec};

    int32_t row0 = 0;
    int64_t counters[4] = {0, 0, 0, 0};
    auto begin = [&](bool first) { // (no dual rows: the covers of this driver carry none)
        for (int k = 0; k < K; k++) {
            const SearchTree t = search_tree(s, d.nfix, k);
            const int lim = first && n[19] > 0 && n[19] < count[k] ? n[19] : count[k];
            for (int i = 0; i < lim; i++) {
                for (size_t e = 0; e < nfix; e++) t.fix[(size_t)i * nfix + e] = n[14] ? c_fix[k][(size_t)i * nfix + e] : (int8_t)-1;
                t.lb[i] = n[14] ? c_lb[k][i] : -INFINITY;
                t.row[i] = -1;
                t.wrow[i] = -1;
                if (first || defect != 2) search_clear_waiting(t, i);
                t.alive[i] = 1;
            }
            search_adopt_scalars(s, t, k, lim, true);
        }
        row0 = 0;
        for (int64_t &c : counters) c = 0;
    };
    begin(true);

    FILE *o = fopen(argv[3], "wb");
    if (!o) return 2;
    const long head = ftell(o);
    int32_t walked = 0, refused = 0;
    put(o, &walked, 1);
    put(o, &refused, 1);
    for (const Round &r : rounds) {
        if (walked == rebegin) begin(false);
        // select: the picks, their blocks, the rows of every tree
        int32_t B = 0, P = 0, waiting = 0;
        for (int k = 0; k < K; k++) {
            const SearchTree t = search_tree(s, d.nfix, k);
            const size_t p = (size_t)k * SEARCH_MAX_WIDTH;
            cnt[k] = search_select_serial(t, width, tol, picks.data() + p);
            int32_t v = 0;
            for (int j = 0; j < cnt[k]; j++) {
                const int i = picks[p + j];
                plev[p + j] = search_pick_levels(t.srow[i], spec, d.nfix, branch_pos_serial(t.fix + (size_t)i * nfix, d.nfix));
                pfirst[p + j] = v;
                v += search_pick_rows(plev[p + j]);
                waiting += plev[p + j] < 0;
            }
            offset[k] = B;
            B += v;
            P += cnt[k];
        }
        if ((long long)row0 + B > row_cap) { // the round is refused: nothing changes
            refused = 1;
            break;
        }
        if (B != r.B) {
            fprintf(stderr, "speculation_driver: round %d stages %d rows, the caller has records for %d\n", walked, B, r.B);
            return 3;
        }
        // stage
        std::vector<int32_t> b_tree(B, -7), b_node(B, -7), b_warm(B, -7);
        std::vector<int8_t> b_fix((size_t)B * nfix);
        for (int k = 0; k < K; k++) {
            if (cnt[k] == 0 && search_running(state[k])) state[k] = search_done_word(inc[k]);
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
        if (P == 0) break; // (no pick: every tree has stopped, and the staging above has said so)
        put(o, &B, 1);
        put(o, &P, 1);
        put(o, b_tree.data(), B);
        put(o, b_node.data(), B);
        put(o, b_warm.data(), B);
        put(o, b_fix.data(), b_fix.size());
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
                if (act == SEARCH_PICK_BRANCHED) {
                    for (int v = 0; v < 2; v++)
                        for (size_t e = 0; e < nfix; e++) fix.at(((size_t)k * node_cap + c + v) * nfix + e) = search_child_fix(fx[e], (int)e, pos, v);
                    if (defect == 1 && L > 0) t.srow[c + 1] = rr + 2;
                }
            }
        }
        counters[0]++;
        counters[1] += B > 0;
        counters[2] += B;
        counters[3] += waiting;
        row0 += B;
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
    put(o, counters, 4);
    fseek(o, head, SEEK_SET);
    put(o, &walked, 1);
    put(o, &refused, 1);
    fclose(o);
    return 0;
}
