// hmpc_stage.h -- the ONE staging table behind every host-pointer entry (include/hmpc.h, include/hmpc_search.h): where each of
// the caller's arrays lies in the block that travels to the device -- inputs first, then outputs, every part at a multiple of
// 256 bytes -- and the host-side copies into and out of that block.  Host only, no HIP: allocation and transfers stay with the
// entries (hmpc_host.h: stage_up / stage_down / stage_each_up / stage_each_down); tests/host/stage_driver.cpp runs the same tables under AddressSanitizer.
#ifndef HMPC_STAGE_H
#define HMPC_STAGE_H

#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "hmpc.h"

struct StagePart {
    size_t bytes;       // what travels; 0: nobody asked for it -- no room (but `pad`) and a null device pointer
    const void *src;    // host array that pack copies into the block (null: the entry fills the part itself, or an output)
    void *dst;          // host array that unpack fills from the block (null: an input, or an output the caller left out)
    size_t row, stride; // rows of `row` bytes: src holds them `stride` bytes apart, unpack can stop after some (0: one piece)
    size_t pad, off;    // room kept behind the bytes, never copied; where the part begins
};

struct StageTable {
    static constexpr int MAX_PARTS = 20;
    StagePart part[MAX_PARTS] = {};
    int n = 0, n_in = 0;                          // parts; the first n_in travel up only, the others come down
    size_t in_end = 0, out_begin = 0, total = 0;  // [0, in_end) is the copy up, [out_begin, total) the copy down; total: all anyone allocates

    StageTable &add(StagePart p, bool up, bool down)
    {
        assert(n < MAX_PARTS && (n == n_in || !up)); // (every table below is shorter: static_assert at the longest; inputs first)
        p.off = total;
        total += (p.bytes + p.pad + 255) / 256 * 256;
        part[n++] = p;
        if (!down) n_in = n, out_begin = total;
        if (up) in_end = total;
        return *this;
    }
    StageTable &in(size_t bytes, const void *src, size_t pad = 0, size_t row = 0, size_t stride = 0) { return add({bytes, src, nullptr, row, stride, pad, 0}, true, false); }
    // read and written by the device: the last part of the copy up and the first of the copy down
    StageTable &inout(size_t bytes, void *both) { return add({bytes, both, both, 0, 0, 0, 0}, true, true); }
    StageTable &out(size_t bytes, void *dst, size_t row = 0, size_t pad = 0) { return add({bytes, nullptr, dst, row, 0, pad, 0}, false, true); }

    size_t end(int i) const { return part[i].off + part[i].bytes; }
    template <class T> T *ptr(int i, char *base) const { return part[i].bytes ? (T *)(base + part[i].off) : nullptr; }
    template <class T> T *at(int i, char *base) const { return (T *)(base + part[i].off); } // a part the entry requires: a pointer even where it is empty
    void pack(char *block) const // every part that has a source into the host block
    {
        for (int i = 0; i < n; i++) {
            const StagePart &p = part[i];
            if (!p.src || !p.bytes) continue;
            if (!p.row || p.stride == p.row) { memcpy(block + p.off, p.src, p.bytes); continue; }
            for (size_t r = 0; r * p.row < p.bytes; r++) memcpy(block + p.off + r * p.row, (const char *)p.src + r * p.stride, p.row);
        }
    }
    void unpack(const char *block, int i, size_t rows = SIZE_MAX) const // part i into its destination: all of it, or its first rows
    {
        const StagePart &p = part[i];
        if (p.dst && p.bytes) memcpy(p.dst, block + p.off, p.row && rows < p.bytes / p.row ? rows * p.row : p.bytes);
    }
};

struct StageDims { size_t nx, nu, nfix, words, n_primal, n_dual; }; // a problem's sizes as the tables need them
constexpr size_t STAGE_F64 = sizeof(double), STAGE_I32 = sizeof(int32_t);

// hmpc_solve_batch: x0 | fix | gathered hand-down (index, primal rows, dual rows: the entry fills them) | the six outputs.  The room
// of a part does not depend on what the caller passes -- x0 has B rows whatever its stride, fix one byte more, primal and dual
// their rows asked for or not -- so a capacity (ensure_staging) holds every batch up to it.
enum { SOLVE_X0, SOLVE_FIX, SOLVE_WIDX, SOLVE_WPRIMAL, SOLVE_WDUAL, SOLVE_OBJ, SOLVE_DOBJ, SOLVE_STATUS, SOLVE_ITERS, SOLVE_PRIMAL, SOLVE_DUAL };
inline StageTable stage_solve(const StageDims &d, size_t B, size_t nwarm, const double *x0, size_t x0_stride, const int8_t *fix, const hmpc_result *out)
{
    const hmpc_result o = out ? *out : hmpc_result{};
    const size_t xrow = d.nx * STAGE_F64, xrows = x0_stride ? B : 1, pb = B * d.n_primal * STAGE_F64, db = B * d.n_dual * STAGE_F64;
    return StageTable().in(xrows * xrow, x0, (B - xrows) * xrow, xrow, x0_stride * STAGE_F64).in(B * d.nfix, fix, 1)
        .in(nwarm ? B * STAGE_I32 : 0, nullptr).in(nwarm * d.n_primal * STAGE_F64, nullptr).in(nwarm * d.n_dual * STAGE_F64, nullptr)
        .out(B * STAGE_F64, o.obj).out(B * STAGE_F64, o.dual_obj).out(B * STAGE_I32, o.status).out(B * STAGE_I32, o.iters)
        .out(o.primal ? pb : 0, o.primal, 0, o.primal ? 0 : pb).out(o.dual ? db : 0, o.dual, 0, o.dual ? 0 : db);
}

// hmpc_certify_batch: x0 | fix | the six members of the records | residuals | verdict (written whether the caller wants it or not)
enum { CERT_X0, CERT_FIX, CERT_OBJ, CERT_DOBJ, CERT_STATUS, CERT_ITERS, CERT_PRIMAL, CERT_DUAL, CERT_RES, CERT_VERDICT };
inline StageTable stage_certify(const StageDims &d, size_t B, const double *x0, size_t x0_stride, const int8_t *fix, const hmpc_result &r, double *residuals,
                                int32_t *verdict)
{
    return StageTable().in((x0_stride ? B : 1) * d.nx * STAGE_F64, x0, 0, d.nx * STAGE_F64, x0_stride * STAGE_F64).in(B * d.nfix, fix)
        .in(B * STAGE_F64, r.obj).in(B * STAGE_F64, r.dual_obj).in(B * STAGE_I32, r.status).in(B * STAGE_I32, r.iters)
        .in(B * d.n_primal * STAGE_F64, r.primal).in(B * d.n_dual * STAGE_F64, r.dual)
        .out(B * HMPC_CERT_COUNT * STAGE_F64, residuals).out(B * STAGE_I32, verdict);
}

// hmpc_branch_batch: a part nobody asks for has no bytes; the child arrays are copied out up to n_children rows, which travels
// wherever they do
enum { BR_FIX, BR_OBJ, BR_STATUS, BR_ITERS, BR_PRIMAL, BR_DUAL, BR_CUTOFF, BR_DOBJ, BR_O_OBJ, BR_O_WORD, BR_O_POS, BR_O_LB2, BR_O_BITS, BR_O_OFFSET, BR_O_N,
       BR_O_CFIX, BR_O_CLB, BR_O_CPARENT, BR_O_CWARM };
static_assert(BR_O_CWARM < StageTable::MAX_PARTS, "the longest table fits");
inline StageTable stage_branch(const StageDims &d, size_t B, const int8_t *fix, const hmpc_result &r, const double *cutoff, bool mark_weak, const hmpc_branch_out &o)
{
    const bool children = o.child_fix || o.child_lb || o.child_parent || o.child_warm;
    return StageTable().in(B * d.nfix, fix).in(B * STAGE_F64, r.obj).in(B * STAGE_I32, r.status).in(B * STAGE_I32, r.iters)
        .in(o.bits ? B * d.n_primal * STAGE_F64 : 0, r.primal).in((o.child_lb2 || o.child_lb) ? B * d.n_dual * STAGE_F64 : 0, r.dual)
        .in(cutoff ? B * STAGE_F64 : 0, cutoff).inout(mark_weak ? B * STAGE_F64 : 0, r.dual_obj)
        .out(o.obj ? B * STAGE_F64 : 0, o.obj).out(o.word ? B * STAGE_I32 : 0, o.word).out(o.pos ? B * STAGE_I32 : 0, o.pos)
        .out(o.child_lb2 ? 2 * B * STAGE_F64 : 0, o.child_lb2).out(o.bits ? B * d.words * sizeof(uint64_t) : 0, o.bits)
        .out(o.child_offset ? B * STAGE_I32 : 0, o.child_offset).out((o.n_children || children) ? STAGE_I32 : 0, o.n_children)
        .out(o.child_fix ? 2 * B * d.nfix : 0, o.child_fix, d.nfix).out(o.child_lb ? 2 * B * STAGE_F64 : 0, o.child_lb, STAGE_F64)
        .out(o.child_parent ? 2 * B * STAGE_I32 : 0, o.child_parent, STAGE_I32).out(o.child_warm ? 2 * B * STAGE_I32 : 0, o.child_warm, STAGE_I32);
}

// hmpc_shift_batch: B leaves of K trees
enum { SH_OWNER, SH_X0, SH_U0, SH_E0, SH_FIX, SH_LB, SH_DUAL, SH_DOBJ, SH_O_FIX, SH_O_LB, SH_O_DUAL, SH_O_DOBJ, SH_O_FLAGS };
inline StageTable stage_shift(const StageDims &d, size_t B, size_t K, const int32_t *owner, const double *x0, const double *u0, const double *e0, const int8_t *fix,
                              const double *lb, const double *dual, const double *dual_obj, int8_t *fix_out, double *lb_out, double *dual_out,
                              double *dual_obj_out, uint8_t *flags)
{
    const size_t nf = B * d.nfix, nd = B * d.n_dual * STAGE_F64, nb = B * STAGE_F64, kx = K * d.nx * STAGE_F64;
    return StageTable().in(B * STAGE_I32, owner).in(kx, x0).in(K * d.nu * STAGE_F64, u0).in(kx, e0).in(nf, fix).in(nb, lb).in(nd, dual).in(nb, dual_obj)
        .out(nf, fix_out).out(nb, lb_out).out(nd, dual_out).out(nb, dual_obj_out).out(B, flags);
}

// hmpc_search_begin: the covers of K trees, compact: offsets (K + 1) | identifiers | bounds of `total` leaves
enum { SB_OFFSET, SB_FIX, SB_LB };
inline StageTable stage_search_begin(const StageDims &d, size_t K, size_t total, const int32_t *offset, const int8_t *fix, const double *lb)
{
    return StageTable().in((K + 1) * STAGE_I32, offset).in(total * d.nfix, fix).in(total * STAGE_F64, lb);
}

// hmpc_search_results: per tree, whatever the caller asks for
enum { SR_COST, SR_U0, SR_X1, SR_SOLVES, SR_LEAVES, SR_STATE, SR_UNCERTIFIED, SR_BINARIES };
inline StageTable stage_search_results(const StageDims &d, size_t K, double *cost, double *u0, double *x1, int8_t *binaries, int32_t *solves, int32_t *leaves,
                                       int32_t *state, int32_t *uncertified)
{
    return StageTable().out(cost ? K * STAGE_F64 : 0, cost).out(u0 ? K * d.nu * STAGE_F64 : 0, u0).out(x1 ? K * d.nx * STAGE_F64 : 0, x1)
        .out(solves ? K * STAGE_I32 : 0, solves).out(leaves ? K * STAGE_I32 : 0, leaves).out(state ? K * STAGE_I32 : 0, state)
        .out(uncertified ? K * STAGE_I32 : 0, uncertified).out(binaries ? K * d.nfix : 0, binaries);
}

// hmpc_search_leaves: where each tree's leaves begin (K) | the N leaves of all trees, whatever the caller asks for
enum { SL_OFFSET, SL_OWNER, SL_LB, SL_DOBJ, SL_DUAL, SL_FIX, SL_HAS_DUAL };
inline StageTable stage_search_leaves(const StageDims &d, size_t K, size_t N, const int32_t *offset, int32_t *owner, int8_t *fix, double *lb, double *dual,
                                      double *dual_obj, uint8_t *has_dual)
{
    return StageTable().in(K * STAGE_I32, offset).out(owner ? N * STAGE_I32 : 0, owner).out(lb ? N * STAGE_F64 : 0, lb).out(dual_obj ? N * STAGE_F64 : 0, dual_obj)
        .out(dual ? N * d.n_dual * STAGE_F64 : 0, dual).out(fix ? N * d.nfix : 0, fix).out(has_dual ? N : 0, has_dual);
}

#endif
