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
#include "hmpc_host.h" // the entries at the end of this file: hmpc_handle, the staging table and its transfers

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

// ---- Host side: the entries of include/hmpc.h (arithmetic: hmpc_branch.h) ------------------------------------------------------
static BranchDims branch_dims_of(const hmpc_handle *h)
{
    const CertProb &c = h->cert; // (the sizes as the caller of hmpc_create stated them)
    return branch_dims(c.nx, c.nu, c.nub, c.T, c.nc, c.ncL, c.nq, c.nr, c.nqT);
}

// everything that can be said about the arguments without the device
static int branch_arguments(const hmpc_handle *h, const int8_t *fix, int32_t B, const hmpc_result *r, int32_t mark_weak, const hmpc_branch_out *out)
{
    if (!fix || !r || !out) return fail(HMPC_EINVAL, "branch: null argument (fix, records and out are required)");
    if (!r->obj || !r->status || !r->iters) return fail(HMPC_EINVAL, "branch: null argument (obj, status and iters of the records are required)");
    if ((out->child_lb2 || out->child_lb) && !r->dual) return fail(HMPC_EINVAL, "branch: the child bounds need the records' dual rows");
    if (out->bits && !r->primal) return fail(HMPC_EINVAL, "branch: the rounded bits need the records' primal rows");
    if (mark_weak && !r->dual_obj) return fail(HMPC_EINVAL, "branch: mark_weak needs the records' dual objectives");
    if ((out->child_fix || out->child_lb || out->child_parent || out->child_warm) && !out->child_offset)
        return fail(HMPC_EINVAL, "branch: the child arrays need child_offset");
    if (!h) return fail(HMPC_EINVAL, "null handle");
    if (h->cert.nub <= 0) return fail(HMPC_EINVAL, "branch: the problem has no binaries (nub == 0)");
    if (B > (1 << 30)) return fail(HMPC_EINVAL, "branch: bad batch size (the children of more than 2^30 nodes have no int32 offsets)");
    return HMPC_OK;
}

// digest, then -- where asked for -- offsets and children, back to back on `stream`: no allocation, no synchronisation
static int hmpc_launch_branch(const BranchDims &d, const BranchArgs &a, hipStream_t st)
{
    const int need = (a.B + BRANCH_WAVES - 1) / BRANCH_WAVES;
    const dim3 grid(need < BRANCH_MAX_GRID ? need : BRANCH_MAX_GRID), block(64 * BRANCH_WAVES);
    const hmpc_branch_out &o = a.out;
    if (o.obj || o.word || o.pos || o.child_lb2 || o.bits || o.child_offset || a.mark_weak) {
        hipLaunchKernelGGL(hmpc_branch_digest_kernel, grid, block, 0, st, d, a);
        HIPCHK(hipGetLastError());
    }
    if (o.child_offset || o.n_children) {
        hipLaunchKernelGGL(hmpc_branch_offsets_kernel, dim3(1), dim3(BRANCH_SCAN_CHUNK), 0, st, d, a);
        HIPCHK(hipGetLastError());
    }
    if (o.child_fix || o.child_lb || o.child_parent || o.child_warm) {
        hipLaunchKernelGGL(hmpc_branch_children_kernel, grid, block, 0, st, d, a);
        HIPCHK(hipGetLastError());
    }
    return HMPC_OK;
}

extern "C" int hmpc_branch_batch_device(hmpc_handle *h, const int8_t *d_fix, int32_t B, const hmpc_result *d_records, const double *d_cutoff,
                                        int32_t warm_base, int32_t mark_weak, const hmpc_branch_out *d_out, void *stream)
{
    g_err.clear();
    if (B < 0) return fail(HMPC_EINVAL, "bad batch size");
    if (h && B == 0) return HMPC_OK; // (an empty batch has no arrays to speak of, and nothing is touched: n_children neither)
    int rc = branch_arguments(h, d_fix, B, d_records, mark_weak, d_out);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const BranchArgs a{B, d_fix, d_records->obj, d_records->dual_obj, d_records->status, d_records->iters, d_records->primal, d_records->dual,
                       d_cutoff, warm_base, mark_weak != 0, *d_out};
    return hmpc_launch_branch(branch_dims_of(h), a, (hipStream_t)stream);
}

// the handle's two staging blocks (as the host-pointer solve uses them, exact fit): inputs up, outputs down; a part nobody asks for has no bytes
extern "C" int hmpc_branch_batch(hmpc_handle *h, const int8_t *fix, int32_t B, const hmpc_result *records, const double *cutoff,
                                 int32_t warm_base, int32_t mark_weak, const hmpc_branch_out *out)
{
    g_err.clear();
    if (B < 0) return fail(HMPC_EINVAL, "bad batch size");
    if (h && B == 0) return HMPC_OK;
    int rc = branch_arguments(h, fix, B, records, mark_weak, out);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const StageTable t = stage_branch(stage_dims(h), (size_t)B, fix, *records, cutoff, mark_weak != 0, *out);
    if ((rc = stage_room(h, t.total, t.total)) || (rc = stage_up(h, t))) return rc;
    char *hs = h->h_stage, *ds = h->d_stage;
    const hmpc_branch_out o{t.ptr<double>(BR_O_OBJ, ds), t.ptr<int32_t>(BR_O_WORD, ds), t.ptr<int32_t>(BR_O_POS, ds), t.ptr<double>(BR_O_LB2, ds),
                            t.ptr<uint64_t>(BR_O_BITS, ds), t.ptr<int32_t>(BR_O_OFFSET, ds), t.ptr<int32_t>(BR_O_N, ds), t.ptr<int8_t>(BR_O_CFIX, ds),
                            t.ptr<double>(BR_O_CLB, ds), t.ptr<int32_t>(BR_O_CPARENT, ds), t.ptr<int32_t>(BR_O_CWARM, ds)};
    const BranchArgs a{B, t.ptr<int8_t>(BR_FIX, ds), t.ptr<double>(BR_OBJ, ds), t.ptr<double>(BR_DOBJ, ds), t.ptr<int32_t>(BR_STATUS, ds),
                       t.ptr<int32_t>(BR_ITERS, ds), t.ptr<double>(BR_PRIMAL, ds), t.ptr<double>(BR_DUAL, ds), t.ptr<double>(BR_CUTOFF, ds), warm_base,
                       mark_weak != 0, o};
    if ((rc = hmpc_launch_branch(branch_dims_of(h), a, nullptr)) || (rc = stage_down(h, t, t.total))) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    int32_t nchild = 0;
    if (t.part[BR_O_N].bytes) std::memcpy(&nchild, hs + t.part[BR_O_N].off, sizeof nchild);
    if (nchild < 0 || (size_t)nchild > 2 * (size_t)B) return fail(HMPC_EDEVICE, "branch: the device returned a number of children outside [0, 2 B]");
    // (rows of the child arrays at and beyond n_children are not written: neither on the device nor here)
    for (int i = t.n_in; i < t.n; i++) t.unpack(hs, i, i >= BR_O_CFIX ? (size_t)nchild : SIZE_MAX);
    return HMPC_OK;
}
