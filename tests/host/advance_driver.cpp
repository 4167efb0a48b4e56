// advance_driver.cpp -- the CPU form of hmpc_search_advance: K trees walked serially through begin -> rounds -> advance, step after
// step, with the per-tree functions of csrc/hmpc_search.h -- what the kernels of csrc/hmpc_search.hip run per lane --, built with
// -fsanitize=address,undefined by tests/test_search_advance_host.py.  It restates none of the arithmetic.  The records of every
// round and the outputs of every shift (shifted identifiers, bounds, flags: the launch between stage and adopt) come from the
// caller, in the order of the staged batch / of the staged leaves; a round or an advance that stages another number than the
// caller has rows for ends the walk with exit code 3.
// defect (for the tests' planted defects, around the header's functions, never in them):
//   1  retain compares with the truncated binary instead of the rounded one
//   2  adopt leaves a slot's wrow as it was
//   3  adopt does not stop a tree one of whose kept leaves the shift dropped
//
//   advance_driver <in> <out>
//   in : int32 nx nu nub T nc ncT nq nr nqT K node_cap row_cap handdown defect has_cover with_rows steps | float64 tol | float64 x0 (K x nx)
//        | if has_cover: int32 count[K], then per tree int8 fix (count x T nub), float64 lb[count]
//        | per step: int32 rounds | per round: int32 width B | float64 obj[B] dual_obj[B] | int32 status[B] iters[B]
//                                                | float64 primal (B x n_primal) dual (B x n_dual)
//                    | int32 has_e0 has_x0_next Bs | float64 e0 (K x nx) if has_e0 | float64 x0_next (K x nx) if has_x0_next
//                    | int8 fix_out (Bs x T nub) | float64 lb_out[Bs] | uint8 flags[Bs]
//   out: per step: int32 rc (0, -1: a tree is running, -3: the kept leaves do not fit the pool; after a refusal the walk ends)
//                  | if rc == 0: int32 B | int32 owner[B] src[B] | float64 lb[B] | int8 fix (B x T nub) | float64 u0 (K x nu) x0 (K x nx)
//                                | int32 cover[K] reopened[K]
//        | per tree: int32 n inc inc_row solves uncertified state | float64 ub unc_lb | int8 fix (n x T nub) | float64 lb[n]
//          | int32 row[n] wrow[n] | uint8 alive[n]
//        | int32 row0
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hmpc_search.h"

template <class T> static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "advance_driver: input too short\n");
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
    const int K = n[9], node_cap = n[10], row_cap = n[11], handdown = n[12], defect = n[13], with_rows = n[15], steps = n[16];
    const double tol = take<double>(f, 1)[0];
    const size_t nfix = (size_t)d.nfix, nodes = (size_t)K * node_cap, rows = (size_t)row_cap, nx = (size_t)d.nx, nu = (size_t)d.nu;
    if (K < 1 || node_cap < 1 || row_cap < 1) return 2;

    // the state, every array exactly as long as the sizes say: an index beyond one is a sanitizer report
    std::vector<int8_t> fix(nodes * nfix, 0);
    std::vector<double> lb(nodes, 0.0), ub(K), unc_lb(K), x0 = take<double>(f, K * nx), p_obj(rows), p_dobj(rows), p_primal(rows * d.n_primal), p_dual(rows * d.n_dual);
    std::vector<int32_t> row(nodes, 0), wrow(nodes, 0), tn(K), inc(K), inc_row(K), solves(K), uncertified(K), state(K), p_status(rows), p_iters(rows);
    std::vector<uint8_t> alive(nodes, 0);
    std::vector<int32_t> picks((size_t)K * SEARCH_MAX_WIDTH), cnt(K), offset(K), word(4);
    SearchState s{K, node_cap, row_cap, fix.data(), lb.data(), row.data(), wrow.data(), alive.data(), tn.data(), inc.data(), inc_row.data(), solves.data(),
                  uncertified.data(), state.data(), ub.data(), unc_lb.data(), x0.data(), p_obj.data(), p_dobj.data(), p_status.data(), p_iters.data(),
                  p_primal.data(), p_dual.data(), picks.data(), cnt.data(), offset.data(), word.data(), nullptr, nullptr, nullptr, nullptr, nullptr};

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
            for (int i = 0; i < count[k]; i++) {
                for (size_t e = 0; e < nfix; e++) t.fix[(size_t)i * nfix + e] = c_fix[(size_t)i * nfix + e];
                t.lb[i] = c_lb[i];
                t.row[i] = n[14] && with_rows ? row0 + i : -1;
                t.wrow[i] = -1;
                t.alive[i] = 1;
            }
            search_adopt_scalars(s, t, k, count[k], true);
            if (n[14] && with_rows) row0 += count[k];
        }
        if (row0 > row_cap) return 2;
    }

    for (int step = 0; step < steps; step++) {
        // ---- the rounds of the step (as tests/host/search_driver.cpp) ----
        const int rounds = take<int32_t>(f, 1)[0];
        for (int q = 0; q < rounds; q++) {
            const std::vector<int32_t> head = take<int32_t>(f, 2);
            const int width = head[0];
            const size_t RB = (size_t)head[1];
            if (width < 1 || width > SEARCH_MAX_WIDTH) return 2;
            const std::vector<double> r_obj = take<double>(f, RB), r_dobj = take<double>(f, RB);
            const std::vector<int32_t> r_status = take<int32_t>(f, RB), r_iters = take<int32_t>(f, RB);
            const std::vector<double> r_primal = take<double>(f, RB * d.n_primal), r_dual = take<double>(f, RB * d.n_dual);
            int32_t B = 0;
            for (int k = 0; k < K; k++) {
                cnt[k] = search_select_serial(search_tree(s, d.nfix, k), width, tol, picks.data() + (size_t)k * SEARCH_MAX_WIDTH);
                offset[k] = B;
                B += cnt[k];
            }
            if ((size_t)B != RB || (long long)row0 + B > row_cap) {
                fprintf(stderr, "advance_driver: step %d round %d stages %d nodes at row %d of %d, the caller has records for %zu\n", step, q, B, row0, row_cap, RB);
                return 3;
            }
            for (int k = 0; k < K; k++)
                if (cnt[k] == 0 && search_running(state[k])) state[k] = search_done_word(inc[k]);
            for (int b = 0; b < B; b++) {
                const size_t r = (size_t)row0 + b;
                p_obj.at(r) = r_obj[b];
                p_dobj.at(r) = r_dobj[b];
                p_status.at(r) = r_status[b];
                p_iters.at(r) = r_iters[b];
                for (int e = 0; e < d.n_primal; e++) p_primal.at(r * d.n_primal + e) = r_primal[(size_t)b * d.n_primal + e];
                for (int e = 0; e < d.n_dual; e++) p_dual.at(r * d.n_dual + e) = r_dual[(size_t)b * d.n_dual + e];
            }
            for (int k = 0; k < K; k++) {
                const SearchTree t = search_tree(s, d.nfix, k);
                for (int j = 0; j < cnt[k]; j++) {
                    const int i = picks[(size_t)k * SEARCH_MAX_WIDTH + j];
                    const int8_t *fx = t.fix + (size_t)i * nfix;
                    const int pos = branch_pos_serial(fx, d.nfix);
                    const int c = *t.n;
                    const int act = search_consume_pick(d, s, t, i, row0 + offset[k] + j, pos, tol);
                    if (act == SEARCH_PICK_STOP) break;
                    if (act == SEARCH_PICK_BRANCHED)
                        for (int v = 0; v < 2; v++)
                            for (size_t e = 0; e < nfix; e++) fix.at(((size_t)k * node_cap + c + v) * nfix + e) = search_child_fix(fx[e], (int)e, pos, v);
                }
            }
            row0 += B;
            (void)handdown;
        }

        // ---- advance ----
        const std::vector<int32_t> head = take<int32_t>(f, 3);
        const size_t Bs = (size_t)head[2];
        const std::vector<double> e0 = head[0] ? take<double>(f, K * nx) : std::vector<double>(K * nx, 0.0);
        const std::vector<double> x0_given = head[1] ? take<double>(f, K * nx) : std::vector<double>();
        std::vector<int8_t> fix_out = take<int8_t>(f, Bs * nfix);
        std::vector<double> lb_out = take<double>(f, Bs);
        std::vector<uint8_t> flags = take<uint8_t>(f, Bs);
        // retain: every tree's kept nodes and their number; offsets: where they begin; the word of the readback
        std::vector<int32_t> keep(nodes), kept(K), first(K), cover(K), reopened(K);
        int32_t B = 0, running = 0;
        for (int k = 0; k < K; k++) {
            const SearchTree t = search_tree(s, d.nfix, k);
            int32_t *mine = keep.data() + (size_t)k * node_cap;
            kept[k] = search_retain_serial(d, s, t, mine);
            if (defect == 1 && search_advances(*t.state)) { // (int) of the binary in place of (int) rint
                const double *u0 = search_incumbent_u0(d, s, t);
                kept[k] = 0;
                for (int i = 0; i < *t.n; i++) {
                    bool agree = t.alive[i] != 0;
                    for (int b = 0; b < d.nub && agree; b++) agree = t.fix[(size_t)i * nfix + b] < 0 || t.fix[(size_t)i * nfix + b] == (int)u0[d.nu - d.nub + b];
                    if (agree) mine[kept[k]++] = i;
                }
            }
            first[k] = B;
            B += kept[k];
            running |= search_running(state[k]);
        }
        int32_t rc = running ? HMPC_EINVAL : B > row_cap ? HMPC_ETOOBIG : HMPC_OK;
        put(o, &rc, 1);
        if (rc) break; // refused: the retain and the scan have written staging only
        if ((size_t)B != Bs) {
            fprintf(stderr, "advance_driver: step %d keeps %d leaves, the caller has shifted %zu\n", step, B, Bs);
            return 3;
        }
        // stage (buffers of exactly B rows)
        std::vector<int32_t> owner(Bs), src(Bs);
        std::vector<int8_t> s_fix(Bs * nfix);
        std::vector<double> s_lb(Bs), u0(K * nu), x0_next(K * nx);
        const SearchShift g{keep.data(), kept.data(), first.data(), nullptr, owner.data(), src.data(), s_fix.data(), s_lb.data(), u0.data(), nullptr, x0_next.data(),
                            fix_out.data(), lb_out.data(), flags.data(), cover.data(), reopened.data()};
        for (int k = 0; k < K; k++) {
            const SearchTree t = search_tree(s, d.nfix, k);
            const bool adv = search_advances(*t.state);
            const double *w = adv ? p_primal.data() + (size_t)*t.inc_row * d.n_primal : nullptr;
            for (size_t e = 0; e < nu; e++) u0[k * nu + e] = search_stage_u0(adv ? w + d.o_u : nullptr, adv, (int)e);
            for (size_t e = 0; e < nx; e++)
                x0_next[k * nx + e] = head[1] ? x0_given[k * nx + e] : search_stage_x0(w, d.nx, adv, x0[k * nx + e], e0[k * nx + e], (int)e);
            for (int j = 0; j < kept[k]; j++) {
                const int i = keep[(size_t)k * node_cap + j];
                const size_t b = (size_t)first[k] + j;
                search_stage_leaf(s, t, g, k, i, b);
                for (size_t e = 0; e < nfix; e++) s_fix.at(b * nfix + e) = t.fix[(size_t)i * nfix + e];
            }
        }
        put(o, &B, 1);
        put(o, owner.data(), Bs);
        put(o, src.data(), Bs);
        put(o, s_lb.data(), Bs);
        put(o, s_fix.data(), Bs * nfix);
        put(o, u0.data(), K * nu);
        // [the shift: fix_out, lb_out, flags are the caller's]
        // adopt
        for (int k = 0; k < K; k++) {
            const SearchTree t = search_tree(s, d.nfix, k);
            const std::vector<int32_t> wrow_before(t.wrow, t.wrow + node_cap);
            bool agreed = true;
            int reop = 0;
            for (int j = 0; j < kept[k]; j++) {
                const size_t b = (size_t)first[k] + j;
                agreed &= search_adopt_leaf(t, g, j, b);
                reop += search_leaf_reopened(s, g, b);
                for (size_t e = 0; e < nfix; e++) fix.at(((size_t)k * node_cap + j) * nfix + e) = fix_out.at(b * nfix + e);
                if (defect == 2) t.wrow[j] = wrow_before[j];
            }
            search_adopt_scalars(s, t, k, kept[k], agreed || defect == 3);
            cover[k] = kept[k];
            reopened[k] = reop;
        }
        x0 = x0_next; // (the same block: s.x0 points at it)
        s.x0 = x0.data();
        row0 = B;
        put(o, x0.data(), K * nx);
        put(o, cover.data(), K);
        put(o, reopened.data(), K);
    }
    fclose(f);
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
    fclose(o);
    return 0;
}
