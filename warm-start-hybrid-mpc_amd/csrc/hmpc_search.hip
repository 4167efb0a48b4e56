// hmpc_search.hip -- the rounds of K device-resident branch-and-bound searches (include/hmpc_search.h).
//
// What a tree does in a round IS hmpc_search.h (and, for the decision about a record, hmpc_branch.h), which compiles for the
// host as well; this file supplies the lane loops, the reductions, the scan and the stores.  Per round, on the caller's stream:
//   select    one workgroup per tree: `width` rounds of an argmin over the keys (lb, index) of the candidates that lie after
//             the last pick (so no list of picked nodes is kept) -- per thread over its nodes, per wave by shuffles, the four
//             waves through LDS.  The picks and their number are written per tree; the tree itself is not touched
//   offsets   ONE workgroup of 1024 threads over the trees in chunks of 1024 with a carry, as hmpc_branch_offsets_kernel: the
//             exclusive scan of the counts -- trees in order, picks of a tree in selection order --, and one word of four for
//             the host: the size B of the round, whether a tree has stopped FAILED / OVERFLOW, whether a node receives a
//             record, whether rows row0 .. row0 + B - 1 fit the pool (if not, stage does nothing: the round is refused)
//   stage     one wavefront per pick: identifier row, the tree's x0 row, the row to hand down, (tree, node); the wavefront of
//             a running tree's first slot marks the tree DONE where it has no pick
//   [the QP kernel writes rows row0 .. row0 + B - 1 of the pool]
//   consume   one wavefront per tree: its picks in selection order, lane 0 carries the serial decisions
//             (search_consume_pick: a COMPLETE pick lowers the cutoff of the next), all lanes compute pos and copy the two
//             identifier rows of a branched node
// and at the end of a step: results (one wavefront per tree: the incumbent's u0, x1 and identifier, the number of leaves) and
// leaves (one wavefront per tree: its alive nodes in list order, 64 at a time by ballot, each copied with the rows it carries).
// Memory bound and small; nothing is staged in LDS but the four partial minima.  Plain C++ stores only: every store is a vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hmpc_search.h"

#define SEARCH_WAVES 4             // wavefronts per workgroup of the stage, consume, results and leaves kernels
#define SEARCH_SELECT_THREADS 256  // threads of a tree's workgroup in select
#define SEARCH_SCAN_CHUNK 1024     // trees per pass of the offsets kernel = its threads
#define SEARCH_MAX_GRID 4096       // workgroups at most (grid-strided beyond)

__global__ void __launch_bounds__(SEARCH_SELECT_THREADS) hmpc_search_select_kernel(const BranchDims d, const SearchState s, const int width, const double tol)
{
    __shared__ double part_lb[SEARCH_SELECT_THREADS / 64];
    __shared__ int part_i[SEARCH_SELECT_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchTree t = search_tree(s, d.nfix, k);
    int cnt = 0;
    if (search_running(*t.state)) { // (the same in every thread)
        const int n = *t.n;
        const double ub = *t.ub;
        double plb = -INFINITY;
        int pi = -1;
        while (cnt < width) {
            double blb = 0.0;
            int bi = -1;
            for (int i = tid; i < n; i += SEARCH_SELECT_THREADS) {
                const double l = t.lb[i];
                if (search_candidate(t.alive[i], l, ub, tol) && search_take(blb, bi, l, i, plb, pi)) { blb = l; bi = i; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ol = __shfl_xor(blb, o);
                const int oi = __shfl_xor(bi, o);
                if (search_take(blb, bi, ol, oi, plb, pi)) { blb = ol; bi = oi; }
            }
            if (lane == 0) { part_lb[wave] = blb; part_i[wave] = bi; }
            __syncthreads();
            blb = 0.0;
            bi = -1;
#pragma unroll
            for (int w = 0; w < SEARCH_SELECT_THREADS / 64; w++)
                if (search_take(blb, bi, part_lb[w], part_i[w], plb, pi)) { blb = part_lb[w]; bi = part_i[w]; }
            __syncthreads(); // (the next round overwrites the partial minima)
            if (bi < 0) break; // (the same in every thread)
            if (tid == 0) s.picks[(size_t)k * SEARCH_MAX_WIDTH + cnt] = bi;
            plb = blb;
            pi = bi;
            cnt++;
        }
    }
    if (tid == 0) s.count[k] = cnt;
}

__global__ void __launch_bounds__(SEARCH_SCAN_CHUNK) hmpc_search_offsets_kernel(const BranchDims d, const SearchState s, const int row0, const int handdown)
{
    __shared__ int32_t totals[SEARCH_SCAN_CHUNK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t carry = 0;
    int bad = 0, warm = 0;
    for (int base = 0; base < s.K; base += SEARCH_SCAN_CHUNK) {
        const int k = base + tid;
        int32_t v = 0;
        if (k < s.K) {
            v = s.count[k];
            bad |= (s.state[k] & (HMPC_SEARCH_FAILED | HMPC_SEARCH_OVERFLOW)) != 0;
            const int32_t *wrow = s.wrow + (size_t)k * s.node_cap;
            for (int j = 0; j < v; j++) warm |= search_warm_index(wrow[s.picks[(size_t)k * SEARCH_MAX_WIDTH + j]], handdown) >= 0;
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
        for (int w = 0; w < SEARCH_SCAN_CHUNK / 64; w++) {
            const int32_t tw = totals[w];
            before += w < wave ? tw : 0;
            chunk += tw;
        }
        if (k < s.K) s.offset[k] = carry + before + incl - v;
        carry += chunk; // (at most K SEARCH_MAX_WIDTH, which hmpc_search_create holds below 2^31)
        __syncthreads(); // (the next chunk overwrites the totals)
    }
    bad = __syncthreads_or(bad);
    warm = __syncthreads_or(warm);
    if (tid == 0) {
        s.word[0] = carry;
        s.word[1] = bad != 0;
        s.word[2] = warm != 0;
        s.word[3] = (long long)row0 + carry <= (long long)s.row_cap;
    }
}

__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_stage_kernel(const BranchDims d, const SearchState s, const int width, const int handdown)
{
    if (!s.word[3]) return; // the round does not fit the pool: nothing changes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long slots = (long long)s.K * width;
    for (long long q = (long long)blockIdx.x * SEARCH_WAVES + wave; q < slots; q += (long long)gridDim.x * SEARCH_WAVES) {
        const int k = (int)(q / width), j = (int)(q % width);
        const int cnt = s.count[k];
        if (j == 0 && cnt == 0 && lane == 0 && search_running(s.state[k])) s.state[k] = search_done_word(s.inc[k]);
        if (j >= cnt) continue; // (the same in every lane)
        const size_t b = (size_t)s.offset[k] + j; // < B <= row_cap - row0
        const int i = s.picks[(size_t)k * SEARCH_MAX_WIDTH + j];
        const int8_t *fix = s.fix + ((size_t)k * s.node_cap + i) * d.nfix;
        for (int e = lane; e < d.nfix; e += 64) s.b_fix[b * d.nfix + e] = fix[e];
        for (int e = lane; e < d.nx; e += 64) s.b_x0[b * d.nx + e] = s.x0[(size_t)k * d.nx + e];
        if (lane == 0) {
            s.b_warm[b] = search_warm_index(s.wrow[(size_t)k * s.node_cap + i], handdown);
            s.b_tree[b] = k;
            s.b_node[b] = i;
        }
    }
}

__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_consume_kernel(const BranchDims d, const SearchState s, const int row0, const double tol)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = blockIdx.x * SEARCH_WAVES + wave; k < s.K; k += gridDim.x * SEARCH_WAVES) {
        const SearchTree t = search_tree(s, d.nfix, k);
        const int cnt = s.count[k];
        const int32_t base = row0 + s.offset[k];
        for (int j = 0; j < cnt; j++) {
            const int i = s.picks[(size_t)k * SEARCH_MAX_WIDTH + j];
            const int8_t *fix = t.fix + (size_t)i * d.nfix;
            const int pos = branch_wave_pos(fix, d.nfix, lane);
            int act = SEARCH_PICK_LEAF, c = 0;
            if (lane == 0) {
                c = *t.n; // where the children go, if there are any
                act = search_consume_pick(d, s, t, i, base + j, pos, tol);
            }
            act = __shfl(act, 0);
            c = __shfl(c, 0);
            if (act == SEARCH_PICK_STOP) break;
            if (act == SEARCH_PICK_BRANCHED) // c + 1 < node_cap: search_consume_pick refuses the pick otherwise
                for (int e = lane; e < d.nfix; e += 64) {
                    const int8_t f = fix[e];
                    t.fix[(size_t)c * d.nfix + e] = search_child_fix(f, e, pos, 0);
                    t.fix[(size_t)(c + 1) * d.nfix + e] = search_child_fix(f, e, pos, 1);
                }
        }
    }
}

struct SearchResults { // per tree, device memory; any member may be null
    double *cost, *u0, *x1;
    int8_t *binaries;
    int32_t *solves, *leaves, *state, *uncertified;
};

__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_results_kernel(const BranchDims d, const SearchState s, const SearchResults r)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = blockIdx.x * SEARCH_WAVES + wave; k < s.K; k += gridDim.x * SEARCH_WAVES) {
        const SearchTree t = search_tree(s, d.nfix, k);
        const int n = *t.n, inc = *t.inc;
        int leaves = 0;
        for (int i = lane; i < n; i += 64) leaves += t.alive[i] != 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) leaves += __shfl_xor(leaves, o);
        const double *w = inc >= 0 ? s.p_primal + (size_t)*t.inc_row * d.n_primal : nullptr;
        if (r.u0)
            for (int e = lane; e < d.nu; e += 64) r.u0[(size_t)k * d.nu + e] = w ? w[d.o_u + e] : NAN;
        if (r.x1)
            for (int e = lane; e < d.nx; e += 64) r.x1[(size_t)k * d.nx + e] = w ? w[d.nx + e] : NAN;
        if (r.binaries)
            for (int e = lane; e < d.nfix; e += 64) r.binaries[(size_t)k * d.nfix + e] = inc >= 0 ? t.fix[(size_t)inc * d.nfix + e] : (int8_t)-1;
        if (lane == 0) {
            if (r.cost) r.cost[k] = inc >= 0 ? *t.ub : INFINITY;
            if (r.solves) r.solves[k] = *t.solves;
            if (r.leaves) r.leaves[k] = leaves;
            if (r.state) r.state[k] = *t.state;
            if (r.uncertified) r.uncertified[k] = *t.uncertified;
        }
    }
}

struct SearchLeaves { // the alive nodes of all trees, compact; device memory; any member but offset may be null
    const int32_t *offset; // K: where tree k's leaves begin (exclusive scan of the results kernel's counts)
    int32_t *owner;
    int8_t *fix;
    double *lb, *dual, *dual_obj;
    uint8_t *has_dual;
};

__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_leaves_kernel(const BranchDims d, const SearchState s, const SearchLeaves o)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = blockIdx.x * SEARCH_WAVES + wave; k < s.K; k += gridDim.x * SEARCH_WAVES) {
        const SearchTree t = search_tree(s, d.nfix, k);
        const int n = *t.n;
        size_t q = (size_t)o.offset[k];
        for (int base = 0; base < n; base += 64) { // (n is the same in every lane: the ballot sees the whole wave)
            const int mine = base + lane;
            unsigned long long m = __ballot(mine < n && t.alive[mine] != 0);
            while (m) { // leaf by leaf in list order, every lane on its rows
                const int i = base + __ffsll((long long)m) - 1;
                m &= m - 1;
                const int32_t row = t.row[i];
                if (o.fix)
                    for (int e = lane; e < d.nfix; e += 64) o.fix[q * d.nfix + e] = t.fix[(size_t)i * d.nfix + e];
                if (o.dual)
                    for (int e = lane; e < d.n_dual; e += 64) o.dual[q * d.n_dual + e] = row >= 0 ? s.p_dual[(size_t)row * d.n_dual + e] : 0.0;
                if (lane == 0) {
                    if (o.owner) o.owner[q] = k;
                    if (o.lb) o.lb[q] = t.lb[i];
                    if (o.dual_obj) o.dual_obj[q] = row >= 0 ? s.p_dual_obj[row] : 0.0;
                    if (o.has_dual) o.has_dual[q] = row >= 0;
                }
                q++;
            }
        }
    }
}

struct SearchBegin { // a step's initial trees, compact (device memory)
    const int32_t *offset; // K + 1, or null: every tree is its root
    const int8_t *fix;
    const double *lb;
    int with_rows;         // leaf j carries pool row j
};

__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_begin_kernel(const BranchDims d, const SearchState s, const SearchBegin g)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = blockIdx.x * SEARCH_WAVES + wave; k < s.K; k += gridDim.x * SEARCH_WAVES) {
        const SearchTree t = search_tree(s, d.nfix, k);
        const int first = g.offset ? g.offset[k] : 0, n = g.offset ? g.offset[k + 1] - first : 1; // <= node_cap (hmpc_search_begin)
        for (int i = 0; i < n; i++)
            for (int e = lane; e < d.nfix; e += 64) t.fix[(size_t)i * d.nfix + e] = g.offset ? g.fix[(size_t)(first + i) * d.nfix + e] : (int8_t)-1;
        for (int i = lane; i < n; i += 64) {
            t.lb[i] = g.offset ? g.lb[first + i] : -INFINITY;
            t.row[i] = g.offset && g.with_rows ? first + i : -1;
            t.wrow[i] = -1;
            t.alive[i] = 1;
        }
        if (lane == 0) {
            *t.n = n;
            *t.ub = INFINITY;
            *t.inc = -1;
            *t.inc_row = -1;
            *t.solves = 0;
            *t.uncertified = 0;
            *t.unc_lb = INFINITY;
            *t.state = 0;
            s.count[k] = 0;
            s.offset[k] = 0;
        }
    }
}
