// hmpc_branch.h -- what branching ONE solved node is (hmpc_branch_batch, include/hmpc.h), item by item.
//
// Plain inline functions that compile for the device (hipcc) and for the host (g++): which binary a node branches on, what
// its record makes of it (branched / complete / pruned / infeasible / failed, and the flags its children inherit), the two
// child bounds, one rounded binary.  The kernels (hmpc_branch.hip) supply the lane loops, the wave reductions, the prefix
// sum and the stores; tests/host/branch_driver.cpp walks the same functions serially under AddressSanitizer.  One
// definition, used by those two and nothing else.
//
// Semantics (reference: warm_start_hmpc/controller.py:13-44 branch_in_time, :395-429 _brancher; branch_and_bound.py:476-489;
// here controller.py branch_in_time / _brancher and tree_consume / fleet_record_round of hmpc_tree.h):
//   pos       1 + the largest j with fix[j] >= 0 (0: none) -- the next binary in (t, i) order after the last fixed one
//   child_lb  obj + nu_ub[pos] (0-branch), obj + nu_lb[pos] (1-branch): ONE float64 addition each -- no product, nothing a
//             compiler could contract -- so host and device agree to the bit
//   word      the decision and the flags, HMPC_BRANCH_* of include/hmpc.h
//   bit j     u_t[nuc + i] > 0.5 of the primal row, j = t nub + i (NaN: false)
// NaN: `obj < cutoff` is false for a NaN objective (or cutoff): the node ends as PRUNED, never as BRANCHED or COMPLETE.
// (tree_consume asks `obj >= cutoff`, which a NaN would pass; no OPTIMAL record of the solver carries one, and the fleet's
// digest path leaves that decision to tree_consume as before.)
#ifndef HMPC_BRANCH_H
#define HMPC_BRANCH_H

#include <math.h>
#include <stdint.h>

#include "hmpc.h"

#ifndef HMPC_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define HMPC_HD __host__ __device__ __forceinline__
#else
#define HMPC_HD inline
#endif
#endif

struct BranchDims {
    int nx, nu, nub, T;
    int nfix, words;        // T nub binaries; 64-bit words that hold one bit each
    int n_primal, n_dual;   // row lengths of hmpc_result.primal / .dual
    int o_lb, o_ub;         // dual row: multipliers of the binaries' lower / upper bounds (nfix each)
    int o_u;                // primal row: u_0 (nu entries per stage, the binaries last)
};

HMPC_HD BranchDims branch_dims(int nx, int nu, int nub, int T, int nc, int ncL, int nq, int nr, int nqT)
{
    BranchDims d;
    d.nx = nx; d.nu = nu; d.nub = nub; d.T = T;
    d.nfix = T * nub;
    d.words = (d.nfix + 63) / 64;
    d.n_primal = (T + 1) * nx + T * nu;
    d.o_lb = (T + 1) * nx + (T - 1) * nc + ncL;
    d.o_ub = d.o_lb + d.nfix;
    d.n_dual = d.o_ub + d.nfix + T * nq + nqT + T * nr;
    d.o_u = (T + 1) * nx;
    return d;
}

// entry j's say on pos (the maximum over all j is pos)
HMPC_HD int branch_pos_item(const int8_t *fix, int j) { return fix[j] >= 0 ? j + 1 : 0; }

HMPC_HD int branch_pos_serial(const int8_t *fix, int nfix)
{
    int pos = 0;
    for (int j = 0; j < nfix; j++) {
        const int p = branch_pos_item(fix, j);
        pos = p > pos ? p : pos;
    }
    return pos;
}

HMPC_HD int32_t branch_word(int32_t status, int32_t iters, double obj, double cutoff, int pos, int nfix)
{
    int32_t w;
    if (status == HMPC_OPTIMAL) {
        w = obj < cutoff ? (pos < nfix ? HMPC_BRANCH_BRANCHED : HMPC_BRANCH_COMPLETE) : HMPC_BRANCH_PRUNED;
        if (iters & HMPC_ITERS_POLISHED) w |= HMPC_BRANCH_VERTEX;
    } else {
        w = status == HMPC_INFEASIBLE ? HMPC_BRANCH_INFEASIBLE : HMPC_BRANCH_FAILED;
    }
    if (iters & HMPC_ITERS_WEAK) w |= HMPC_BRANCH_WEAK;
    if (iters & HMPC_ITERS_UNCERTIFIED) w |= HMPC_BRANCH_UNCERTIFIED;
    if (iters & HMPC_ITERS_HANDED) w |= HMPC_BRANCH_HANDED;
    return w;
}

// the bound of the v-branch (v = 0: the upper bound of binary pos comes down to 0, v = 1: its lower bound goes up to 1);
// dual: the node's dual row, read only where the bound is finite
HMPC_HD double branch_child_lb(const BranchDims &d, int32_t status, double obj, const double *dual, int pos, int v)
{
    if (status != HMPC_OPTIMAL || pos >= d.nfix) return INFINITY;
    return obj + dual[(v ? d.o_lb : d.o_ub) + pos];
}

// whether `bits` is computed for the node (else zero): its record may be handed down and it has a binary left
HMPC_HD bool branch_has_bits(const BranchDims &d, int32_t word, int pos) { return (word & HMPC_BRANCH_VERTEX) && pos < d.nfix; }

HMPC_HD bool branch_bit(const BranchDims &d, const double *primal, int j)
{
    return primal[d.o_u + (j / d.nub) * d.nu + (d.nu - d.nub) + j % d.nub] > 0.5;
}

HMPC_HD int32_t branch_child_warm(int32_t word, int32_t warm_base, int32_t b) { return (word & HMPC_BRANCH_VERTEX) ? warm_base + b : -1; }

#endif // HMPC_BRANCH_H
