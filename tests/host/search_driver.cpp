// search_driver.cpp -- the CPU form of the rounds of hmpc_search: a serial walk over K trees with the per-tree functions of
// csrc/hmpc_search.h (and, through them, csrc/hmpc_branch.h) -- what the kernels of csrc/hmpc_search.hip do with a workgroup
// argmin, a scan and lane loops --, built with -fsanitize=address,undefined by tests/test_search_host.py.  It restates none of
// the arithmetic.  The records of every round come from the caller (oracle-solved or synthetic), in the order of the batch
// the round stages; a round that stages another number of nodes than it has records for ends the walk with exit code 3 (a last round of
// no records says that the search must have ended there).
// defect (for the tests' planted defects, around the header's functions, never in them):
//   1  consume compares every pick of a round with the cutoff the round began with
//   2  select lets the last of equal bounds win
//
//   search_driver <in> <out>
//   in : int32 nx nu nub T nc ncT nq nr nqT K node_cap width handdown defect has_cover rounds | float64 tol
//        | if has_cover: int32 count[K], then per tree int8 fix (count x T nub), float64 lb[count]
//        | per round: int32 B | float64 obj[B] dual_obj[B] | int32 status[B] iters[B] | float64 primal (B x n_primal) dual (B x n_dual)
//   out: int32 rounds walked | per round: int32 B, tree[B], node[B], warm[B]
//        | per tree: int32 n inc inc_row solves uncertified state | float64 ub unc_lb | int8 fix (n x T nub) | float64 lb[n]
//          | int32 row[n] wrow[n] | uint8 alive[n]
//        | int32 rows | float64 dual_obj[rows] of the pool
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hmpc_search.h"

template <class T> static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "search_driver: input too short\n");
        exit(2);
    }
    return v;
}

template <class T> static void put(FILE *f, const T *p, size_t n)
{
    if (n && fwrite(p, sizeof(T), n, f) != n) exit(2);
}

struct Round {
    int32_t B;
    std::vector<double> obj, dual_obj, primal, dual;
    std::vector<int32_t> status, iters;
};

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> n = take<int32_t>(f, 16);
    const BranchDims d = branch_dims(n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8]);
    const int K = n[9], node_cap = n[10], width = n[11], handdown = n[12], defect = n[13];
    const double tol = take<double>(f, 1)[0];
    const size_t nfix = (size_t)d.nfix, nodes = (size_t)K * node_cap;
    if (width < 1 || width > SEARCH_MAX_WIDTH) return 2;

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
    size_t rows = 0;
    for (Round &r : rounds) {
        r.B = take<int32_t>(f, 1)[0];
        const size_t B = (size_t)r.B;
        r.obj = take<double>(f, B);
        r.dual_obj = take<double>(f, B);
        r.status = take<int32_t>(f, B);
        r.iters = take<int32_t>(f, B);
        r.primal = take<double>(f, B * d.n_primal);
        r.dual = take<double>(f, B * d.n_dual);
        rows += B;
    }
    fclose(f);

    // the state, every array exactly as long as the sizes say: an index beyond one is a sanitizer report
    std::vector<int8_t> fix(nodes * nfix, 0);
    std::vector<double> lb(nodes, 0.0), ub(K), unc_lb(K), p_obj(rows), p_dobj(rows), p_primal(rows * d.n_primal), p_dual(rows * d.n_dual);
    std::vector<int32_t> row(nodes, 0), wrow(nodes, 0), tn(K), inc(K), inc_row(K), solves(K), uncertified(K), state(K), p_status(rows), p_iters(rows);
    std::vector<uint8_t> alive(nodes, 0);
    std::vector<int32_t> picks((size_t)K * SEARCH_MAX_WIDTH), cnt(K), offset(K), word(4);
    SearchState s{K, node_cap, (int)rows, fix.data(), lb.data(), row.data(), wrow.data(), alive.data(), tn.data(), inc.data(), inc_row.data(), solves.data(),
                  uncertified.data(), state.data(), ub.data(), unc_lb.data(), nullptr, p_obj.data(), p_dobj.data(), p_status.data(), p_iters.data(),
                  p_primal.data(), p_dual.data(), picks.data(), cnt.data(), offset.data(), word.data(), nullptr, nullptr, nullptr, nullptr, nullptr};

    // begin (no dual rows: the covers of this driver carry none)
    for (int k = 0; k < K; k++) {
        const SearchTree t = search_tree(s, d.nfix, k);
        for (int i = 0; i < count[k]; i++) {
            for (size_t e = 0; e < nfix; e++) t.fix[(size_t)i * nfix + e] = n[14] ? c_fix[k][(size_t)i * nfix + e] : (int8_t)-1;
            t.lb[i] = n[14] ? c_lb[k][i] : -INFINITY;
            t.row[i] = -1;
            t.wrow[i] = -1;
            t.alive[i] = 1;
        }
        *t.n = count[k];
        *t.ub = INFINITY;
        *t.inc = -1;
        *t.inc_row = -1;
        *t.solves = 0;
        *t.uncertified = 0;
        *t.unc_lb = INFINITY;
        *t.state = 0;
    }

    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    const long head = ftell(o);
    int32_t walked = 0;
    put(o, &walked, 1);
    int32_t row0 = 0;
    for (const Round &r : rounds) {
        // select
        int32_t B = 0;
        for (int k = 0; k < K; k++) {
            const SearchTree t = search_tree(s, d.nfix, k);
            int32_t *mine = picks.data() + (size_t)k * SEARCH_MAX_WIDTH;
            cnt[k] = search_select_serial(t, width, tol, mine);
            if (defect == 2 && search_running(*t.state)) { // among equal bounds the last index first
                std::vector<int> cand;
                for (int i = 0; i < *t.n; i++)
                    if (search_candidate(t.alive[i], t.lb[i], *t.ub, tol)) cand.push_back(i);
                for (size_t a = 0; a < cand.size(); a++)
                    for (size_t b = a + 1; b < cand.size(); b++)
                        if (t.lb[cand[b]] < t.lb[cand[a]] || (t.lb[cand[b]] == t.lb[cand[a]] && cand[b] > cand[a])) std::swap(cand[a], cand[b]);
                for (int j = 0; j < cnt[k]; j++) mine[j] = cand[j];
            }
            offset[k] = B;
            B += cnt[k];
        }
        if (B != r.B) {
            fprintf(stderr, "search_driver: round %d stages %d nodes, the caller has records for %d\n", walked, B, r.B);
            return 3;
        }
        // stage
        std::vector<int32_t> b_tree(B), b_node(B), b_warm(B);
        for (int k = 0; k < K; k++) {
            if (cnt[k] == 0 && search_running(state[k])) state[k] = search_done_word(inc[k]);
            for (int j = 0; j < cnt[k]; j++) {
                const int i = picks[(size_t)k * SEARCH_MAX_WIDTH + j];
                b_tree.at(offset[k] + j) = k;
                b_node.at(offset[k] + j) = i;
                b_warm.at(offset[k] + j) = search_warm_index(wrow[(size_t)k * node_cap + i], handdown);
            }
        }
        if (B == 0) break; // (a last round without records: every tree has stopped, and the staging above has said so)
        put(o, &B, 1);
        put(o, b_tree.data(), B);
        put(o, b_node.data(), B);
        put(o, b_warm.data(), B);
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
            const double ub0 = *t.ub;
            for (int j = 0; j < cnt[k]; j++) {
                const int i = picks[(size_t)k * SEARCH_MAX_WIDTH + j];
                const int8_t *fx = t.fix + (size_t)i * nfix;
                const int pos = branch_pos_serial(fx, d.nfix);
                const int c = *t.n;
                const double ub_now = *t.ub;
                const int32_t inc_before = *t.inc;
                if (defect == 1) *t.ub = ub0;
                const int act = search_consume_pick(d, s, t, i, row0 + offset[k] + j, pos, tol);
                if (defect == 1 && *t.inc == inc_before) *t.ub = ub_now;
                if (act == SEARCH_PICK_STOP) break;
                if (act == SEARCH_PICK_BRANCHED)
                    for (int v = 0; v < 2; v++)
                        for (size_t e = 0; e < nfix; e++) fix.at(((size_t)k * node_cap + c + v) * nfix + e) = search_child_fix(fx[e], (int)e, pos, v);
            }
        }
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
    }
    put(o, &row0, 1);
    put(o, p_dobj.data(), (size_t)row0);
    fseek(o, head, SEEK_SET);
    put(o, &walked, 1);
    fclose(o);
    return 0;
}
