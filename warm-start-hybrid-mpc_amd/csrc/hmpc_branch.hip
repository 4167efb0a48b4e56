// hmpc_branch.hip -- branching a batch of solved nodes on the device (hmpc_branch_batch, include/hmpc.h).
//
// What branching one node IS lives in hmpc_branch.h and compiles for the host as well; this file supplies the lane loops, the
// wave reductions, the prefix sum and the stores.  Three small kernels, launched back to back on the caller's stream:
//   digest    one wavefront per node, four nodes per workgroup, grid-strided: the lanes stride over the identifier for pos
//             (wave maximum), over the binaries of the primal row for the rounded bits (one 64-bit ballot per word), lane 0
//             writes objective, word, pos and the two child bounds, and -- mark_weak -- -inf into the dual objective of a
//             weak node; where offsets are asked for it leaves the node's number of children (2 / 0) in child_offset
//   offsets   ONE workgroup of 1024 threads over the batch in chunks of BRANCH_SCAN_CHUNK = 1024 nodes: an exclusive prefix sum
//             in place (wave scan by shuffles, the sixteen wave totals through LDS, a running carry between chunks), the
//             total into n_children.  Deterministic and ordered -- children of node b before those of b' > b -- which an
//             atomic slot counter would not be
//   children  one wavefront per node: the node's decision again from the same functions (it reads the identifier anyway, to
//             copy it), then two rows: identifier with fix[pos] = 0 / 1, bound, parent, row to hand down
// Memory: per node nfix bytes of identifier, three words of the record, two multipliers and -- for the bits of a vertex node
// -- nfix strided doubles of the primal row are read; 32 + 8 ceil(nfix / 64) bytes and, per branched node, 2 (nfix + 16) bytes
// are written.  The work is memory bound and small; nothing is staged.  Plain C++ stores only: every store is a vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hmpc_branch.h"

#define BRANCH_WAVES 4          // nodes (waves) per workgroup of the digest and children kernels
#define BRANCH_SCAN_CHUNK 1024  // nodes per pass of the offsets kernel = its threads
#define BRANCH_MAX_GRID 2048    // workgroups at most (grid-strided beyond)

struct BranchArgs {
    int B;
    const int8_t *fix;       // B x nfix
    const double *obj;       // records
    double *dual_obj;        //   (written where mark_weak)
    const int32_t *status, *iters;
    const double *primal, *dual;
    const double *cutoff;    // B, or null: +inf
    int32_t warm_base, mark_weak;
    hmpc_branch_out out;
};

static __device__ __forceinline__ int branch_wave_max(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// pos of node b's identifier: every lane ends with the maximum
static __device__ __forceinline__ int branch_wave_pos(const int8_t *fix, int nfix, int lane)
{
    int pos = 0;
    for (int j = lane; j < nfix; j += 64) {
        const int p = branch_pos_item(fix, j);
        pos = p > pos ? p : pos;
    }
    return branch_wave_max(pos);
}

__global__ void __launch_bounds__(64 * BRANCH_WAVES) hmpc_branch_digest_kernel(const BranchDims d, const BranchArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = blockIdx.x * BRANCH_WAVES + wave; b < a.B; b += gridDim.x * BRANCH_WAVES) {
        const int pos = branch_wave_pos(a.fix + (size_t)b * d.nfix, d.nfix, lane);
        const int32_t status = a.status[b], iters = a.iters[b];
        const double obj = a.obj[b], cutoff = a.cutoff ? a.cutoff[b] : INFINITY;
        const int32_t word = branch_word(status, iters, obj, cutoff, pos, d.nfix);
        if (a.out.bits) {
            const bool has = branch_has_bits(d, word, pos);
            const double *w = a.primal + (size_t)b * d.n_primal;
            for (int k = 0; k < d.words; k++) { // (trip count and `has` are the same in every lane: the ballot sees the whole wave)
                const int j = k * 64 + lane;
                const bool bit = has && j < d.nfix && branch_bit(d, w, j);
                const unsigned long long m = __ballot(bit);
                if (lane == 0) a.out.bits[(size_t)b * d.words + k] = (uint64_t)m;
            }
        }
        if (lane == 0) {
            if (a.out.obj) a.out.obj[b] = obj;
            if (a.out.word) a.out.word[b] = word;
            if (a.out.pos) a.out.pos[b] = pos;
            if (a.out.child_lb2) {
                const double *dl = a.dual + (size_t)b * d.n_dual;
                a.out.child_lb2[2 * (size_t)b] = branch_child_lb(d, status, obj, dl, pos, 0);
                a.out.child_lb2[2 * (size_t)b + 1] = branch_child_lb(d, status, obj, dl, pos, 1);
            }
            if (a.out.child_offset) a.out.child_offset[b] = (word & HMPC_BRANCH_BRANCHED) ? 2 : 0; // (the offsets kernel sums these in place)
            if (a.mark_weak && (iters & HMPC_ITERS_WEAK)) a.dual_obj[b] = -INFINITY;
        }
    }
}

// Exclusive prefix sum of the nodes' numbers of children.  With child_offset they are what the digest kernel left there
// (summed in place); without it (n_children alone is asked for) every thread works its node's count out by itself.
__global__ void __launch_bounds__(BRANCH_SCAN_CHUNK) hmpc_branch_offsets_kernel(const BranchDims d, const BranchArgs a)
{
    __shared__ int32_t totals[BRANCH_SCAN_CHUNK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t carry = 0;
    for (int base = 0; base < a.B; base += BRANCH_SCAN_CHUNK) {
        const int b = base + tid;
        int32_t v = 0;
        if (b < a.B) {
            if (a.out.child_offset) {
                v = a.out.child_offset[b];
            } else {
                const int pos = branch_pos_serial(a.fix + (size_t)b * d.nfix, d.nfix);
                v = (branch_word(a.status[b], a.iters[b], a.obj[b], a.cutoff ? a.cutoff[b] : INFINITY, pos, d.nfix) & HMPC_BRANCH_BRANCHED) ? 2 : 0;
            }
        }
        int32_t incl = v; // inclusive scan within the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) totals[wave] = incl;
        __syncthreads();
        int32_t before = 0, chunk = 0;
#pragma unroll
        for (int w = 0; w < BRANCH_SCAN_CHUNK / 64; w++) {
            const int32_t t = totals[w];
            before += w < wave ? t : 0;
            chunk += t;
        }
        if (b < a.B && a.out.child_offset) a.out.child_offset[b] = carry + before + incl - v;
        carry += chunk;
        __syncthreads(); // (the next chunk overwrites the totals)
    }
    if (tid == 0 && a.out.n_children) a.out.n_children[0] = carry;
}

__global__ void __launch_bounds__(64 * BRANCH_WAVES) hmpc_branch_children_kernel(const BranchDims d, const BranchArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = blockIdx.x * BRANCH_WAVES + wave; b < a.B; b += gridDim.x * BRANCH_WAVES) {
        const int8_t *fix = a.fix + (size_t)b * d.nfix;
        const int pos = branch_wave_pos(fix, d.nfix, lane);
        const int32_t status = a.status[b];
        const double obj = a.obj[b];
        const int32_t word = branch_word(status, a.iters[b], obj, a.cutoff ? a.cutoff[b] : INFINITY, pos, d.nfix);
        if (!(word & HMPC_BRANCH_BRANCHED)) continue; // (the same in every lane)
        const size_t row = (size_t)a.out.child_offset[b]; // < 2 B - 1: the sum of at most B twos, this node's included
        if (a.out.child_fix)
            for (int j = lane; j < d.nfix; j += 64) {
                const int8_t f = fix[j];
                a.out.child_fix[row * d.nfix + j] = j == pos ? (int8_t)0 : f;
                a.out.child_fix[(row + 1) * d.nfix + j] = j == pos ? (int8_t)1 : f;
            }
        if (lane < 2) { // lane v writes the scalars of the v-branch
            const size_t c = row + lane;
            if (a.out.child_lb) a.out.child_lb[c] = branch_child_lb(d, status, obj, a.dual + (size_t)b * d.n_dual, pos, lane);
            if (a.out.child_parent) a.out.child_parent[c] = b;
            if (a.out.child_warm) a.out.child_warm[c] = branch_child_warm(word, a.warm_base, b);
        }
    }
}
