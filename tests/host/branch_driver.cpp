// branch_driver.cpp -- the CPU form of hmpc_branch_batch: a serial loop over the per-node functions of csrc/hmpc_branch.h, a
// serial prefix sum and scatter (what the three kernels of csrc/hmpc_branch.hip do with lanes, shuffles and a ballot), built
// with -fsanitize=address,undefined by tests/test_branch_host.py.  It restates none of the arithmetic.
// Beside it, the project's own host definition of a branch: every node whose identifier is a chronological prefix goes
// through the fleet's host logic (csrc/hmpc_tree.h) -- recorded once from its record (fleet_record_round) and once from the
// digest computed here (fleet_record_round_digest), consumed by tree_consume -- and the two trees must agree to the bit
// (exit 5 otherwise); the children of the first are written out for the test to hold against the scatter.
//
//   branch_driver <in> <out>
//   in : int32 nx nu nub T nc ncT nq nr nqT B has_cutoff warm_base mark_weak | int8 fix (B x T nub) | float64 obj[B] dual_obj[B]
//        | int32 status[B] iters[B] | float64 primal (B x n_primal) dual (B x n_dual) | float64 cutoff[B] if has_cutoff
//   out: float64 obj[B] child_lb2[2B] | int32 word[B] pos[B] | uint64 bits (B x words) | int32 child_offset[B] n_children
//        | int8 child_fix (n x T nub) | float64 child_lb[n] | int32 child_parent[n] child_warm[n] | float64 dual_obj[B]
//        | int32 tree_count[B] (-1: not a prefix or a NaN objective, -2: tree_consume refused a failed node) | int8 tree_fix (2B x T nub)
//        | float64 tree_lb[2B] | int32 tree_warm[2B]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hmpc_branch.h"
#include "hmpc_tree.h"

template <class T> static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "branch_driver: input too short\n");
        exit(2);
    }
    return v;
}

template <class T> static void put(FILE *f, const std::vector<T> &v)
{
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
}

static bool same_tree(const FleetTree &a, const FleetTree &b)
{
    if (a.n != b.n || a.fix != b.fix || a.row != b.row || a.wrow != b.wrow || a.alive != b.alive || a.depth != b.depth || a.inc != b.inc ||
        a.inc_row != b.inc_row || a.solves != b.solves || a.uncertified != b.uncertified || a.rounded != b.rounded)
        return false;
    return std::memcmp(a.lb.data(), b.lb.data(), a.lb.size() * sizeof(double)) == 0 && std::memcmp(&a.ub, &b.ub, sizeof(double)) == 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> n = take<int32_t>(f, 13);
    const BranchDims d = branch_dims(n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8]);
    const FleetDims fd = fleet_dims(n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8]);
    if (fd.nfix != d.nfix || fd.n_primal != d.n_primal || fd.n_dual != d.n_dual || fd.o_lb != d.o_lb) {
        fprintf(stderr, "branch_driver: hmpc_branch.h and hmpc_tree.h disagree on the layout\n");
        return 4;
    }
    const size_t B = (size_t)n[9], nfix = (size_t)d.nfix, words = (size_t)d.words;
    const int32_t warm_base = n[11];
    const bool mark_weak = n[12] != 0;
    // every row in a block of its own, exactly as long as the layout says: an index beyond a row is a sanitizer report
    std::vector<std::vector<int8_t>> fix;
    for (size_t b = 0; b < B; b++) fix.push_back(take<int8_t>(f, nfix));
    const std::vector<double> obj = take<double>(f, B);
    std::vector<double> dobj = take<double>(f, B);
    const std::vector<int32_t> status = take<int32_t>(f, B), iters = take<int32_t>(f, B);
    std::vector<std::vector<double>> primal, dual;
    for (size_t b = 0; b < B; b++) primal.push_back(take<double>(f, d.n_primal));
    for (size_t b = 0; b < B; b++) dual.push_back(take<double>(f, d.n_dual));
    const std::vector<double> cutoff = n[10] ? take<double>(f, B) : std::vector<double>(B, INFINITY);
    fclose(f);

    // digest
    std::vector<double> o_obj(B), o_lb2(2 * B);
    std::vector<int32_t> o_word(B), o_pos(B), o_off(B), count(B);
    std::vector<uint64_t> o_bits(B * words, 0);
    for (size_t b = 0; b < B; b++) {
        const int pos = branch_pos_serial(fix[b].data(), d.nfix);
        const int32_t word = branch_word(status[b], iters[b], obj[b], cutoff[b], pos, d.nfix);
        o_obj[b] = obj[b];
        o_word[b] = word;
        o_pos[b] = pos;
        o_lb2[2 * b] = branch_child_lb(d, status[b], obj[b], dual[b].data(), pos, 0);
        o_lb2[2 * b + 1] = branch_child_lb(d, status[b], obj[b], dual[b].data(), pos, 1);
        if (branch_has_bits(d, word, pos))
            for (int j = 0; j < d.nfix; j++)
                if (branch_bit(d, primal[b].data(), j)) o_bits[b * words + j / 64] |= (uint64_t)1 << (j % 64);
        count[b] = (word & HMPC_BRANCH_BRANCHED) ? 2 : 0;
        if (mark_weak && (iters[b] & HMPC_ITERS_WEAK)) dobj[b] = -INFINITY;
    }
    // offsets
    int32_t total = 0;
    for (size_t b = 0; b < B; b++) { o_off[b] = total; total += count[b]; }
    // children
    std::vector<std::vector<int8_t>> c_fix((size_t)total, std::vector<int8_t>(nfix));
    std::vector<double> c_lb((size_t)total);
    std::vector<int32_t> c_parent((size_t)total), c_warm((size_t)total);
    for (size_t b = 0; b < B; b++) {
        if (!(o_word[b] & HMPC_BRANCH_BRANCHED)) continue;
        for (int v = 0; v < 2; v++) {
            const size_t c = (size_t)o_off[b] + v;
            for (int j = 0; j < d.nfix; j++) c_fix.at(c)[j] = j == o_pos[b] ? (int8_t)v : fix[b][j];
            c_lb.at(c) = branch_child_lb(d, status[b], obj[b], dual[b].data(), o_pos[b], v);
            c_parent.at(c) = (int32_t)b;
            c_warm.at(c) = branch_child_warm(o_word[b], warm_base, (int32_t)b);
        }
    }

    // the fleet's host logic on the same nodes: one tree per node, the node its only leaf
    std::vector<int32_t> t_count(B, -1), t_warm(2 * B, 0);
    std::vector<int8_t> t_fix(2 * B * nfix, 0);
    std::vector<double> t_lb(2 * B, 0.0);
    const std::vector<double> x0(d.nx, 0.0);
    for (size_t b = 0; b < B; b++) {
        const int pos = o_pos[b];
        bool prefix = true;
        for (int j = 0; j < pos; j++) prefix = prefix && fix[b][j] >= 0;
        if (!prefix || obj[b] != obj[b]) continue; // (tree_key and depth mean prefixes; `obj >= cutoff` lets a NaN through, `obj < cutoff` does not)
        std::vector<FleetTree> one(1), two(1);
        for (std::vector<FleetTree> *tr : {&one, &two}) {
            FleetTree &t = (*tr)[0];
            tree_reset_cold(t, d.nfix);
            tree_begin_step(t, x0.data(), d.nx);
            t.fix = fix[b];
            t.depth[0] = (int16_t)pos;
            t.ub = cutoff[b]; // (tree_consume prunes against ub - tol)
        }
        const std::vector<FleetLaunch> launch{{0, pos}};
        std::vector<int32_t> weak;
        const int h1 = fleet_record_round(one, launch, fd, warm_base + (int32_t)b, 1, fix[b].data(), &obj[b], &status[b], &iters[b], dual[b].data() + fd.o_lb,
                                          (size_t)fd.n_dual, primal[b].data(), (size_t)fd.n_primal, weak);
        const int h2 = fleet_record_round_digest(two, launch, fd, warm_base + (int32_t)b, 1, fix[b].data(), &o_obj[b], &o_word[b], &o_pos[b], &o_lb2[2 * b],
                                                 &o_bits[b * words], words);
        if (h1 != h2 || weak.size() != (size_t)((iters[b] & HMPC_ITERS_WEAK) != 0)) { fprintf(stderr, "branch_driver: node %zu: the two records differ\n", b); return 5; }
        const std::vector<int> picks{0};
        const int r1 = tree_consume(one[0], picks, d.nfix, 0.0), r2 = tree_consume(two[0], picks, d.nfix, 0.0);
        if (r1 != r2 || !same_tree(one[0], two[0])) { fprintf(stderr, "branch_driver: node %zu: the digest's tree is not the records' tree\n", b); return 5; }
        if (r1 == 2) { t_count[b] = -2; continue; }
        if (r1 != 0) return 5;
        const FleetTree &t = one[0];
        t_count[b] = t.n - 1;
        for (int c = 1; c < t.n && c < 3; c++) {
            std::memcpy(&t_fix[(2 * b + c - 1) * nfix], &t.fix[(size_t)c * nfix], nfix);
            t_lb[2 * b + c - 1] = t.lb[c];
            t_warm[2 * b + c - 1] = t.wrow[c];
        }
    }

    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    put(o, o_obj); put(o, o_lb2); put(o, o_word); put(o, o_pos); put(o, o_bits); put(o, o_off);
    put(o, std::vector<int32_t>{total});
    for (const auto &row : c_fix) put(o, row);
    put(o, c_lb); put(o, c_parent); put(o, c_warm); put(o, dobj);
    put(o, t_count); put(o, t_fix); put(o, t_lb); put(o, t_warm);
    fclose(o);
    return 0;
}
