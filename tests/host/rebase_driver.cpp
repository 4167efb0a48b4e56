// rebase_driver.cpp -- the CPU form of hmpc_search_rebase: K trees walked serially through begin and a list of operations -- rounds,
// re-bases, advances -- with the per-tree functions of csrc/hmpc_search.h -- what the kernels of csrc/hmpc_search.hip run per lane
// --, built with -fsanitize=address,undefined and -ffp-contract=off by tests/rebase_reference.py.  It restates none of the
// arithmetic.  The records of every round and the outputs of every shift come from the caller, as in advance_driver.cpp; a round or
// an advance that stages another number than the caller has rows for ends the walk with exit code 3.  The dual pool exists twice
// and swaps with every re-base, as on the device (an advance's shifted rows are the caller's business: its pool stays).
// defect (for the tests' planted defects, around the header's functions, never in them):
//   1  the bound is moved from the leaf's lb instead of its row's dual objective
//   2  the new row keeps the dual objective of the row it was copied from
//   3  a FAILED / OVERFLOW tree keeps its leaves
//
//   rebase_driver <in> <out>
//   in : int32 nx nu nub T nc ncT nq nr nqT K node_cap row_cap handdown defect has_cover with_rows ops | float64 tol | float64 x0 (K x nx)
//        | if has_cover: int32 count[K], then per tree int8 fix (count x T nub), float64 lb[count] and, if with_rows, float64 dual
//          (count x n_dual), dual_obj[count]
//        | per op: int32 kind
//            0 (round):   int32 width B | float64 obj[B] dual_obj[B] | int32 status[B] iters[B] | float64 primal (B x n_primal) dual (B x n_dual)
//            1 (advance): int32 has_e0 has_x0_next Bs | float64 e0 (K x nx) if has_e0 | float64 x0_next (K x nx) if has_x0_next
//                         | int8 fix_out (Bs x T nub) | float64 lb_out[Bs] | uint8 flags[Bs]
//            2 (rebase):  float64 x0_new (K x nx)
//   out: per advance / rebase: int32 rc (0; -1: a tree is running (advance only); -3: the kept leaves do not fit the pool -- a refusal
//                  changes nothing and the walk goes on)
//                  | if rc == 0: int32 B | int32 owner[B] src[B] | float64 lb[B] | int32 cover[K] reopened[K] | float64 x0 (K x nx)
//                                | rebase only: float64 lb_out[B] | float64 dual (B x n_dual) dual_obj[B]: rows 0 .. B - 1 of the pool
//                  | per tree: int32 n inc inc_row solves uncertified state | float64 ub unc_lb | int8 fix (n x T nub) | float64 lb[n]
//                    | int32 row[n] wrow[n] | uint8 alive[n]
//        | int32 row0
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "hmpc_search.h"

template <class T> static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "rebase_driver: input too short\n");
        exit(2);
    }
    return v;
}

template <class T> static void put(FILE *f, const T *p, size_t n)
{
    if (n && fwrite(p, sizeof(T), n, f) != n) exit(2);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    FILE *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    const std::vector<int32_t> n = take<int32_t>(f, 17);
    const BranchDims d = branch_dims(n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8]);
    const int K = n[9], node_cap = n[10], row_cap = n[11], defect = n[13], with_rows = n[15], ops = n[16];
    const double tol = take<double>(f, 1)[0];
    const size_t nfix = (size_t)d.nfix, nodes = (size_t)K * node_cap, rows = (size_t)row_cap, nx = (size_t)d.nx, nu = (size_t)d.nu, nd = (size_t)d.n_dual;
    if (K < 1 || node_cap < 1 || row_cap < 1) return 2;

    // the state, every array exactly as long as the sizes say: an index beyond one is a sanitizer report.  Both dual pools end
    // with the row of zeros a leaf without a row is moved from.
    std::vector<int8_t> fix(nodes * nfix, 0);
    std::vector<double> lb(nodes, 0.0), ub(K), unc_lb(K), x0 = take<double>(f, K * nx), p_obj(rows), p_primal(rows * d.n_primal);
    std::vector<double> p_dual((rows + 1) * nd, 0.0), p_dobj(rows + 1, 0.0), q_dual((rows + 1) * nd, 0.0), q_dobj(rows + 1, 0.0);
    std::vector<int32_t> row(nodes, 0), wrow(nodes, 0), srow(nodes, 7), sleft(nodes, 7), tn(K), inc(K), inc_row(K), solves(K), uncertified(K), state(K), p_status(rows), p_iters(rows);
    std::vector<uint8_t> alive(nodes, 0);
    std::vector<int32_t> picks((size_t)K * SEARCH_MAX_WIDTH), cnt(K), offset(K), word(4);
    SearchState s{K, node_cap, row_cap, fix.data(), lb.data(), row.data(), wrow.data(), alive.data(), tn.data(), inc.data(), inc_row.data(), solves.data(),
                  uncertified.data(), state.data(), ub.data(), unc_lb.data(), x0.data(), p_obj.data(), p_dobj.data(), p_status.data(), p_iters.data(),
                  p_primal.data(), p_dual.data(), picks.data(), cnt.data(), offset.data(), word.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                  srow.data(), sleft.data(), nullptr, nullptr, 0};

    // begin
    int32_t row0 = 0;
    {
        std::vector<int32_t> count(K, 1);
        if (n[14]) count = take<int32_t>(f, K);
        for (int k = 0; k < K; k++) {
            if (count[k] < 0 || count[k] > node_cap) return 2;
            const SearchTree t = search_tree(s, d.nfix, k);
            const std::vector<int8_t> c_fix = n[14] ? take<int8_t>(f, (size_t)count[k] * nfix) : std::vector<int8_t>(nfix, (int8_t)-1);
            const std::vector<double> c_lb = n[14] ? take<double>(f, count[k]) : std::vector<double>(1, -INFINITY);
            const bool carries = n[14] && with_rows;
            if (carries) {
                if ((size_t)row0 + count[k] > rows) return 2;
                const std::vector<double> c_dual = take<double>(f, (size_t)count[k] * nd), c_dobj = take<double>(f, count[k]);
                for (size_t e = 0; e < c_dual.size(); e++) p_dual.at((size_t)row0 * nd + e) = c_dual[e];
                for (size_t e = 0; e < c_dobj.size(); e++) p_dobj.at((size_t)row0 + e) = c_dobj[e];
            }
            for (int i = 0; i < count[k]; i++) {
                for (size_t e = 0; e < nfix; e++) t.fix[(size_t)i * nfix + e] = c_fix[(size_t)i * nfix + e];
                t.lb[i] = c_lb[i];
                t.row[i] = carries ? row0 + i : -1;
                t.wrow[i] = -1;
                search_clear_waiting(t, i);
                t.alive[i] = 1;
            }
            search_adopt_scalars(s, t, k, count[k], true);
            if (carries) row0 += count[k];
        }
    }

    for (int op = 0; op < ops; op++) {
        const int kind = take<int32_t>(f, 1)[0];
        if (kind == 0) {
            // ---- a round (as tests/host/search_driver.cpp) ----
            const std::vector<int32_t> head = take<int32_t>(f, 2);
            const int width = head[0];
            const size_t RB = (size_t)head[1];
            if (width < 1 || width > SEARCH_MAX_WIDTH) return 2;
            const std::vector<double> r_obj = take<double>(f, RB), r_dobj = take<double>(f, RB);
            const std::vector<int32_t> r_status = take<int32_t>(f, RB), r_iters = take<int32_t>(f, RB);
            const std::vector<double> r_primal = take<double>(f, RB * d.n_primal), r_dual = take<double>(f, RB * nd);
            int32_t B = 0;
            for (int k = 0; k < K; k++) {
                cnt[k] = search_select_serial(search_tree(s, d.nfix, k), width, tol, picks.data() + (size_t)k * SEARCH_MAX_WIDTH);
                offset[k] = B;
                B += cnt[k];
            }
            if ((size_t)B != RB || (long long)row0 + B > row_cap) {
                fprintf(stderr, "rebase_driver: op %d stages %d nodes at row %d of %d, the caller has records for %zu\n", op, B, row0, row_cap, RB);
                return 3;
            }
            for (int k = 0; k < K; k++)
                if (cnt[k] == 0 && search_running(state[k])) state[k] = search_done_word(inc[k]);
            for (int b = 0; b < B; b++) {
                const size_t r = (size_t)row0 + b;
                p_obj.at(r) = r_obj[b];
                s.p_dual_obj[r] = r_dobj[b];
                p_status.at(r) = r_status[b];
                p_iters.at(r) = r_iters[b];
                for (int e = 0; e < d.n_primal; e++) p_primal.at(r * d.n_primal + e) = r_primal[(size_t)b * d.n_primal + e];
                for (size_t e = 0; e < nd; e++) s.p_dual[r * nd + e] = r_dual[(size_t)b * nd + e];
            }
            for (int k = 0; k < K; k++) {
                const SearchTree t = search_tree(s, d.nfix, k);
                for (int j = 0; j < cnt[k]; j++) {
                    const int i = picks[(size_t)k * SEARCH_MAX_WIDTH + j];
                    const int8_t *fx = t.fix + (size_t)i * nfix;
                    const int pos = branch_pos_serial(fx, d.nfix);
                    const int c = *t.n;
                    const int act = search_consume_waiting(d, s, t, i, row0 + offset[k] + j, 0, pos, tol);
                    if (act == SEARCH_PICK_STOP) break;
                    if (act == SEARCH_PICK_BRANCHED)
                        for (int v = 0; v < 2; v++)
                            for (size_t e = 0; e < nfix; e++) fix.at(((size_t)k * node_cap + c + v) * nfix + e) = search_child_fix(fx[e], (int)e, pos, v);
                }
            }
            row0 += B;
            continue;
        }
        if (kind != 1 && kind != 2) return 2;
        const bool rebase = kind == 2;

        // ---- the inputs of the boundary ----
        size_t Bs = 0;
        std::vector<double> e0(K * nx, 0.0), x0_given;
        std::vector<int8_t> fix_out;
        std::vector<double> lb_out;
        std::vector<uint8_t> flags;
        bool given = rebase;
        if (rebase) {
            x0_given = take<double>(f, K * nx);
        } else {
            const std::vector<int32_t> head = take<int32_t>(f, 3);
            Bs = (size_t)head[2];
            if (head[0]) e0 = take<double>(f, K * nx);
            if (head[1]) x0_given = take<double>(f, K * nx);
            given = head[1] != 0;
            fix_out = take<int8_t>(f, Bs * nfix);
            lb_out = take<double>(f, Bs);
            flags = take<uint8_t>(f, Bs);
        }
        // retain: every tree's kept nodes and their number; offsets: where they begin; the word of the readback
        std::vector<int32_t> keep(nodes), kept(K), first(K), cover(K), reopened(K);
        int32_t B = 0, running = 0;
        for (int k = 0; k < K; k++) {
            const SearchTree t = search_tree(s, d.nfix, k);
            int32_t *mine = keep.data() + (size_t)k * node_cap;
            kept[k] = rebase ? search_rebase_retain_serial(t, mine) : search_retain_serial(d, s, t, mine);
            if (rebase && defect == 3 && !search_rebases(*t.state)) {
                kept[k] = 0;
                for (int i = 0; i < *t.n; i++)
                    if (t.alive[i]) mine[kept[k]++] = i;
            }
            first[k] = B;
            B += kept[k];
            running |= !rebase && search_running(state[k]);
        }
        int32_t rc = running ? HMPC_EINVAL : B > row_cap ? HMPC_ETOOBIG : HMPC_OK;
        put(o, &rc, 1);
        if (rc == HMPC_OK) {
            if (!rebase && (size_t)B != Bs) {
                fprintf(stderr, "rebase_driver: op %d keeps %d leaves, the caller has shifted %zu\n", op, B, Bs);
                return 3;
            }
            Bs = (size_t)B;
            // stage (buffers of exactly B rows)
            std::vector<int32_t> owner(Bs), src(Bs);
            std::vector<int8_t> s_fix(Bs * nfix);
            std::vector<double> s_lb(Bs), u0(K * nu), x0_next(K * nx);
            if (rebase) {
                lb_out.assign(Bs, 0.0);
                flags.assign(Bs, 0);
            }
            const SearchShift g{keep.data(), kept.data(), first.data(), nullptr, owner.data(), src.data(), s_fix.data(), s_lb.data(), u0.data(), nullptr, x0_next.data(),
                                rebase ? s_fix.data() : fix_out.data(), lb_out.data(), flags.data(), cover.data(), reopened.data()};
            for (int k = 0; k < K; k++) {
                const SearchTree t = search_tree(s, d.nfix, k);
                const bool adv = !rebase && search_advances(*t.state);
                const double *w = adv ? p_primal.data() + (size_t)*t.inc_row * d.n_primal : nullptr;
                for (size_t e = 0; e < nu; e++) u0[k * nu + e] = search_stage_u0(adv ? w + d.o_u : nullptr, adv, (int)e);
                for (size_t e = 0; e < nx; e++)
                    x0_next[k * nx + e] = given ? x0_given[k * nx + e] : search_stage_x0(w, d.nx, adv, x0[k * nx + e], e0[k * nx + e], (int)e);
                for (int j = 0; j < kept[k]; j++) {
                    const int i = keep[(size_t)k * node_cap + j];
                    const size_t b = (size_t)first[k] + j;
                    search_stage_leaf(s, t, g, k, i, b);
                    for (size_t e = 0; e < nfix; e++) s_fix.at(b * nfix + e) = t.fix[(size_t)i * nfix + e];
                }
            }
            // rebase-rows: row b of the other pool is the row the leaf carried, its dual objective and the leaf's bound are moved
            // [an advance: the shift -- fix_out, lb_out, flags are the caller's]
            if (rebase)
                for (size_t b = 0; b < Bs; b++) {
                    const size_t r = (size_t)src[b], k = (size_t)owner[b];
                    for (size_t e = 0; e < nd; e++) q_dual.at(b * nd + e) = s.p_dual[r * nd + e];
                    const double obj = search_rebase_obj(s.p_dual + r * nd, defect == 1 ? s_lb[b] : s.p_dual_obj[r], x0_next.data() + k * nx, x0.data() + k * nx, d.nx);
                    lb_out[b] = search_rebase_bound(s_lb[b], obj, &flags[b]);
                    q_dobj.at(b) = defect == 2 ? s.p_dual_obj[r] : obj;
                }
            // adopt
            for (int k = 0; k < K; k++) {
                const SearchTree t = search_tree(s, d.nfix, k);
                bool agreed = true;
                int reop = 0, nodes_k = kept[k];
                for (int j = 0; j < kept[k]; j++) {
                    const size_t b = (size_t)first[k] + j;
                    agreed &= search_adopt_leaf(t, g, j, b);
                    reop += search_leaf_reopened(s, g, b);
                    for (size_t e = 0; e < nfix; e++) fix.at(((size_t)k * node_cap + j) * nfix + e) = g.fix_out[b * nfix + e];
                }
                if (rebase && !search_rebases(*t.state) && defect != 3) {
                    nodes_k = search_rebase_root(t);
                    for (size_t e = 0; e < nfix; e++) fix.at((size_t)k * node_cap * nfix + e) = SEARCH_ROOT_FIX;
                }
                search_adopt_scalars(s, t, k, nodes_k, agreed || rebase);
                cover[k] = kept[k];
                reopened[k] = reop;
            }
            x0 = x0_next; // (the same block: s.x0 points at it)
            s.x0 = x0.data();
            if (rebase) { // the pools swap
                std::swap(p_dual, q_dual);
                std::swap(p_dobj, q_dobj);
                s.p_dual = p_dual.data();
                s.p_dual_obj = p_dobj.data();
            }
            row0 = B;
            put(o, &B, 1);
            put(o, owner.data(), Bs);
            put(o, src.data(), Bs);
            put(o, s_lb.data(), Bs);
            put(o, cover.data(), K);
            put(o, reopened.data(), K);
            put(o, x0.data(), K * nx);
            if (rebase) {
                put(o, lb_out.data(), Bs);
                put(o, p_dual.data(), Bs * nd);
                put(o, p_dobj.data(), Bs);
            }
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
            for (size_t i = 0; rc == HMPC_OK && i < m; i++)
                if (t.srow[i] != -1 || t.sleft[i] != 0) {
                    fprintf(stderr, "rebase_driver: op %d leaves a waiting record on node %zu of tree %d\n", op, i, k);
                    return 4;
                }
        }
    }
    fclose(f);
    put(o, &row0, 1);
    fclose(o);
    return 0;
}
