// hmpc_search.hip -- the rounds of K device-resident branch-and-bound searches (include/hmpc_search.h).
//
// What a tree does in a round IS hmpc_search.h (and, for the decision about a record, hmpc_branch.h), which compiles for the
// host as well; this file supplies the lane loops, the reductions, the scan and the stores.  Per round, on the caller's stream:
//   select    one workgroup per tree: `width` rounds of an argmin over the keys (lb, index) of the candidates that lie after
//             the last pick (so no list of picked nodes is kept) -- per thread over its nodes, per wave by shuffles, the four
//             waves through LDS.  The picks and their number are written per tree; the tree itself is not touched.
//             (include/hmpc_search_anytime.h: under another rule the key's first entry is -index or index, the same loop; under a
//             budget the rounds are min(width, budget left), and a tree without budget looks for one candidate it does not pick)
//   blocks    (speculation depth > 0 only) one wavefront per pick: pos of its identifier, hence the levels of the block it
//             emits -- the node and its descendants through its next binaries, S(L) rows --, or -1 where its record waits
//   offsets   ONE workgroup of 1024 threads over the trees in chunks of 1024 with a carry, as hmpc_branch_offsets_kernel: the
//             exclusive scan of the EMITTED ROWS -- trees in order, blocks of a tree in selection order --, and one word of six
//             for the host: the size B of the round, whether a tree has stopped FAILED / OVERFLOW, whether a node receives a
//             record, whether rows row0 .. row0 + B - 1 fit the pool (if not, stage does nothing: the round is refused), the
//             number of picks P and how many of them are served from waiting records
//   stage     one wavefront per emitted row: identifier row (the pick's, with the binaries of the row's pre-order index set),
//             the tree's x0 row, the row to hand down, (tree, node); the wavefront of a running tree's first slot marks the
//             tree DONE where it has no pick (out of BUDGET where select found it with candidates and no budget left)
//   [the QP kernel writes rows row0 .. row0 + B - 1 of the pool]
//   consume   one wavefront per tree: its picks in selection order, lane 0 carries the serial decisions
//             (search_consume_waiting: a COMPLETE pick lowers the cutoff of the next; the record is the pick's waiting one or
//             the first row of its block), all lanes compute pos and copy the two identifier rows of a branched node
// and at the end of a step: results (one wavefront per tree: the incumbent's u0, x1 and identifier, the number of leaves) and
// leaves (one wavefront per tree: its alive nodes in list order, 64 at a time by ballot, each copied with the rows it carries),
// or, without leaving the device, advance: retain -> offsets -> stage -> the node shift (hmpc_launch_shift) -> adopt, further down;
// and rebase (the trees carried to a neighbouring state of the same stage): the same kernels under a compile-time switch around
// rebase-rows, one wavefront per kept leaf.
// Memory bound and small; nothing is staged in LDS but the four partial minima.  Plain C++ stores only: every store is a vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <memory>

#include "hmpc_search.h"
#include "hmpc_host.h" // the entries at the end of this file: hmpc_handle (and branch_dims_of, hmpc_branch.hip), the staging table and its transfers

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
    int cnt = 0, open = 0;
    if (search_running(*t.state)) { // (the same in every thread)
        const int n = *t.n;
        const double ub = *t.ub;
        // the rule's key takes the bound's place (best-first: it IS the bound); under a budget the tree stages `limit` picks, and
        // with none left it still looks for ONE candidate, which it does not pick: search_select_anytime
        const int order = search_tree_rule(s.rule, *t.inc), limit = search_pick_limit(width, s.budget1, *t.solves);
        const int probe = limit > 0 ? limit : 1;
        double plb = -INFINITY;
        int pi = -1;
        while (cnt < probe) {
            double blb = 0.0;
            int bi = -1;
            for (int i = tid; i < n; i += SEARCH_SELECT_THREADS) {
                const double b = t.lb[i], l = search_rule_key(order, b, i);
                if (search_candidate(t.alive[i], b, ub, tol) && search_take(blb, bi, l, i, plb, pi)) { blb = l; bi = i; }
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
            if (tid == 0 && cnt < limit) s.picks[(size_t)k * SEARCH_MAX_WIDTH + cnt] = bi;
            plb = blb;
            pi = bi;
            cnt++;
        }
        open = cnt > limit; // (only with limit == 0: a candidate and no budget)
        cnt = cnt < limit ? cnt : limit;
    }
    if (tid == 0) {
        s.count[k] = cnt;
        if (s.open) s.open[k] = open;
    }
}

// hmpc_search_set_budget: the trees a budget had stopped run again
__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_reopen_kernel(const SearchState s)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < s.K; k += gridDim.x * blockDim.x)
        if (search_budget_stopped(s.state[k])) s.state[k] = 0;
}

// hmpc_search_bounds: one wavefront per tree, the minimum of its leaves' bounds and the number of its candidates by shuffles
// (a minimum is exact: the result does not depend on the order of the reduction)
__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_bounds_kernel(const BranchDims d, const SearchState s, const double tol, double *lower, double *upper,
                                                                               int32_t *open)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = blockIdx.x * SEARCH_WAVES + wave; k < s.K; k += gridDim.x * SEARCH_WAVES) {
        const SearchTree t = search_tree(s, d.nfix, k);
        const int n = *t.n;
        const double ub = *t.ub;
        double lo = INFINITY;
        int32_t cand = 0;
        for (int i = lane; i < n; i += 64) {
            const uint8_t a = t.alive[i];
            const double l = t.lb[i];
            if (a) lo = search_bound_min(lo, l);
            cand += search_candidate(a, l, ub, tol);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = search_bound_min(lo, __shfl_xor(lo, o));
            cand += __shfl_xor(cand, o);
        }
        if (lane == 0) {
            lower[k] = search_bound_min(lo, *t.unc_lb);
            upper[k] = ub;
            open[k] = cand;
        }
    }
}

// Exclusive scan of v over the SEARCH_SCAN_CHUNK threads of the workgroup, in thread order; chunk: the sum over all of them.
// totals: SEARCH_SCAN_CHUNK / 64 entries of LDS, free again when the call returns.
static __device__ __forceinline__ int32_t search_chunk_scan(int32_t v, int32_t *totals, int lane, int wave, int32_t &chunk)
{
    int32_t incl = v; // inclusive scan within the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) totals[wave] = incl;
    __syncthreads();
    int32_t before = 0;
    chunk = 0;
#pragma unroll
    for (int w = 0; w < SEARCH_SCAN_CHUNK / 64; w++) {
        const int32_t tw = totals[w];
        before += w < wave ? tw : 0;
        chunk += tw;
    }
    __syncthreads(); // (the next call overwrites the totals)
    return before + incl - v;
}

// the levels of every pick's block (speculation depth > 0: they depend on pos, which takes a wavefront)
__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_blocks_kernel(const BranchDims d, const SearchState s, const int width)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long slots = (long long)s.K * width;
    for (long long q = (long long)blockIdx.x * SEARCH_WAVES + wave; q < slots; q += (long long)gridDim.x * SEARCH_WAVES) {
        const int k = (int)(q / width), j = (int)(q % width);
        if (j >= s.count[k]) continue; // (the same in every lane)
        const size_t o = (size_t)k * s.node_cap + s.picks[(size_t)k * SEARCH_MAX_WIDTH + j];
        const int pos = branch_wave_pos(s.fix + o * d.nfix, d.nfix, lane);
        if (lane == 0) s.plev[(size_t)k * SEARCH_MAX_WIDTH + j] = search_pick_levels(s.srow[o], s.spec, d.nfix, pos);
    }
}

__global__ void __launch_bounds__(SEARCH_SCAN_CHUNK) hmpc_search_offsets_kernel(const BranchDims d, const SearchState s, const int row0, const int handdown)
{
    __shared__ int32_t totals[SEARCH_SCAN_CHUNK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t carry = 0, picks = 0, waiting = 0;
    int bad = 0, warm = 0;
    for (int base = 0; base < s.K; base += SEARCH_SCAN_CHUNK) {
        const int k = base + tid;
        int32_t v = 0;
        if (k < s.K) {
            const int cnt = s.count[k];
            bad |= (s.state[k] & (HMPC_SEARCH_FAILED | HMPC_SEARCH_OVERFLOW)) != 0;
            const size_t o = (size_t)k * s.node_cap, p = (size_t)k * SEARCH_MAX_WIDTH;
            for (int j = 0; j < cnt; j++) { // the rows the tree emits: block after block in selection order
                const int i = s.picks[p + j];
                // (depth 0: a block is the node, whatever its pos -- the blocks kernel has not run)
                const int lev = s.spec ? s.plev[p + j] : search_pick_levels(s.srow[o + i], 0, d.nfix, 0);
                s.plev[p + j] = lev;
                s.pfirst[p + j] = v;
                v += search_pick_rows(lev);
                waiting += lev < 0;
                warm |= lev >= 0 && search_warm_index(s.wrow[o + i], handdown) >= 0;
            }
            picks += cnt;
        }
        int32_t chunk;
        const int32_t before = search_chunk_scan(v, totals, lane, wave, chunk);
        if (k < s.K) s.offset[k] = carry + before;
        carry += chunk; // (emitted rows: at most K SEARCH_MAX_WIDTH S(depth), which hmpc_search_set_speculation holds below 2^31)
    }
    bad = __syncthreads_or(bad);
    warm = __syncthreads_or(warm);
    int32_t chunk;
    search_chunk_scan(picks, totals, lane, wave, chunk); // (the sums over the workgroup: every thread has the trees tid, tid + 1024, ...)
    picks = chunk;
    search_chunk_scan(waiting, totals, lane, wave, chunk);
    waiting = chunk;
    if (tid == 0) {
        s.word[0] = carry;
        s.word[1] = bad != 0;
        s.word[2] = warm != 0;
        s.word[3] = (long long)row0 + carry <= (long long)s.row_cap;
        s.word[4] = picks;
        s.word[5] = waiting;
    }
}

__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_stage_kernel(const BranchDims d, const SearchState s, const int width, const int handdown)
{
    if (!s.word[3]) return; // the round does not fit the pool: nothing changes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int most = search_block_rows(s.spec); // rows of a pick's block at most: one wavefront for each of them
    const long long slots = (long long)s.K * width * most;
    for (long long w = (long long)blockIdx.x * SEARCH_WAVES + wave; w < slots; w += (long long)gridDim.x * SEARCH_WAVES) {
        const int q = (int)(w % most), j = (int)((w / most) % width), k = (int)(w / most / width);
        const int cnt = s.count[k];
        if (q == 0 && j == 0 && cnt == 0 && lane == 0 && search_running(s.state[k])) s.state[k] = search_stop_word(s.inc[k], s.open ? s.open[k] : 0);
        if (j >= cnt) continue; // (the same in every lane)
        const int lev = s.plev[(size_t)k * SEARCH_MAX_WIDTH + j];
        if (q >= search_pick_rows(lev)) continue; // the pick's record waits, or its block is shorter
        const size_t b = (size_t)s.offset[k] + s.pfirst[(size_t)k * SEARCH_MAX_WIDTH + j] + q; // < B <= row_cap - row0
        const int i = s.picks[(size_t)k * SEARCH_MAX_WIDTH + j];
        const int8_t *fix = s.fix + ((size_t)k * s.node_cap + i) * d.nfix;
        int bits = 0;
        const int m = search_block_path(lev, q, &bits);
        const int pos = m ? branch_wave_pos(fix, d.nfix, lane) : 0; // (row 0 is the node itself: nothing is set)
        for (int e = lane; e < d.nfix; e += 64) s.b_fix[b * d.nfix + e] = search_block_fix(fix[e], e, pos, m, bits);
        for (int e = lane; e < d.nx; e += 64) s.b_x0[b * d.nx + e] = s.x0[(size_t)k * d.nx + e];
        if (lane == 0) {
            s.b_warm[b] = q == 0 ? search_warm_index(s.wrow[(size_t)k * s.node_cap + i], handdown) : -1; // (a descendant's parent rides in this launch)
            s.b_tree[b] = k;
            s.b_node[b] = q == 0 ? i : -1;
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
                const size_t p = (size_t)k * SEARCH_MAX_WIDTH + j;
                act = search_consume_waiting(d, s, t, i, search_pick_row(t, i, base + s.pfirst[p]), search_pick_left(t, i, s.plev[p]), pos, tol);
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
            search_clear_waiting(t, i);
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

// ---- advance: retain -> offsets -> stage -> [hmpc_launch_shift] -> adopt (arithmetic: hmpc_search.h) ---------------------------
// retain   one wavefront per tree: its nodes 64 at a time, each lane tests its own node's stage-0 entries against the incumbent's
//          input; the kept nodes go into the tree's index list in list order (ballot, rank = kept lanes below), with their number
//          (REBASE: every alive node of a tree that takes part -- search_rebases, search_rebase_retained)
template <bool REBASE>
__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_retain_kernel(const BranchDims d, const SearchState s, const SearchShift g)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = blockIdx.x * SEARCH_WAVES + wave; k < s.K; k += gridDim.x * SEARCH_WAVES) {
        const SearchTree t = search_tree(s, d.nfix, k);
        int cnt = 0;
        if (REBASE ? search_rebases(*t.state) : search_advances(*t.state)) { // (the same in every lane)
            const int n = *t.n;
            const double *u0 = REBASE ? nullptr : search_incumbent_u0(d, s, t);
            int32_t *keep = g.keep + (size_t)k * s.node_cap;
            for (int base = 0; base < n; base += 64) {
                const int mine = base + lane;
                bool kept = mine < n;
                if constexpr (REBASE) kept = kept && search_rebase_retained(t.alive[mine < n ? mine : 0]);
                else kept = kept && t.alive[mine] != 0 && search_retained(d, t.fix + (size_t)mine * d.nfix, u0);
                const unsigned long long m = __ballot(kept);
                if (kept) keep[cnt + __popcll(m & ((1ull << lane) - 1))] = mine; // < n <= node_cap
                cnt += __popcll(m);
            }
        }
        if (lane == 0) g.kept[k] = cnt;
    }
}

// offsets  ONE workgroup: where every tree's kept leaves begin (the scan of the rounds' offsets kernel), and the word the host reads
//          (REBASE: a running tree is no refusal)
template <bool REBASE>
__global__ void __launch_bounds__(SEARCH_SCAN_CHUNK) hmpc_search_advance_offsets_kernel(const SearchState s, const SearchShift g)
{
    __shared__ int32_t totals[SEARCH_SCAN_CHUNK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t carry = 0;
    int running = 0;
    for (int base = 0; base < s.K; base += SEARCH_SCAN_CHUNK) {
        const int k = base + tid;
        int32_t v = 0;
        if (k < s.K) {
            v = g.kept[k];
            running |= search_running(s.state[k]);
        }
        int32_t chunk;
        const int32_t before = search_chunk_scan(v, totals, lane, wave, chunk);
        if (k < s.K) g.first[k] = carry + before;
        carry += chunk; // (at most K node_cap, which hmpc_search_create holds below 2^31)
    }
    running = __syncthreads_or(running);
    if (tid == 0) {
        g.word[0] = carry;
        g.word[1] = !REBASE && running != 0;
        g.word[2] = carry <= s.row_cap;
    }
}

// stage    one wavefront per tree: what the shift reads -- per kept leaf its tree, the row it carries, its bound and its identifier,
//          per tree the applied input and the next state (given != 0: the caller's, already in place)
//          (REBASE: the kept leaves only -- no input is applied, and the new state is always the caller's)
template <bool REBASE>
__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_advance_stage_kernel(const BranchDims d, const SearchState s, const SearchShift g, const int given)
{
    if (g.word[1] || !g.word[2]) return; // refused: a tree is running, or the leaves do not fit the pool
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = blockIdx.x * SEARCH_WAVES + wave; k < s.K; k += gridDim.x * SEARCH_WAVES) {
        const SearchTree t = search_tree(s, d.nfix, k);
        if constexpr (!REBASE) {
            const bool adv = search_advances(*t.state);
            const double *w = adv ? s.p_primal + (size_t)*t.inc_row * d.n_primal : nullptr;
            for (int e = lane; e < d.nu; e += 64) g.u0[(size_t)k * d.nu + e] = search_stage_u0(adv ? w + d.o_u : nullptr, adv, e);
            if (!given)
                for (int e = lane; e < d.nx; e += 64)
                    g.x0_next[(size_t)k * d.nx + e] = search_stage_x0(w, d.nx, adv, s.x0[(size_t)k * d.nx + e], g.e0[(size_t)k * d.nx + e], e);
        }
        const int cnt = g.kept[k];
        const size_t first = (size_t)g.first[k]; // first + cnt <= B <= row_cap
        const int32_t *keep = g.keep + (size_t)k * s.node_cap;
        for (int j = lane; j < cnt; j += 64) search_stage_leaf(s, t, g, k, keep[j], first + j);
        for (int j = 0; j < cnt; j++) {
            const int8_t *fix = t.fix + (size_t)keep[j] * d.nfix;
            for (int e = lane; e < d.nfix; e += 64) g.fix[(first + j) * d.nfix + e] = fix[e];
        }
    }
}

// adopt    one wavefront per tree: the shifted leaves are the tree (it reads the staging and the shift's outputs only, never the
//          slab it overwrites); cover and reopened by shuffles; a kept leaf the shift dropped stops the tree
//          (REBASE: the identifiers are the staged ones, copied; a tree that does not take part becomes its root; no tree fails)
template <bool REBASE>
__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_adopt_kernel(const BranchDims d, const SearchState s, const SearchShift g)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = blockIdx.x * SEARCH_WAVES + wave; k < s.K; k += gridDim.x * SEARCH_WAVES) {
        const SearchTree t = search_tree(s, d.nfix, k);
        const int cnt = g.kept[k]; // <= the tree's nodes <= node_cap
        const size_t first = (size_t)g.first[k];
        const int8_t *ident = REBASE ? g.fix : g.fix_out;
        int dropped = 0, reop = 0, n = cnt;
        for (int j = lane; j < cnt; j += 64) {
            dropped |= !search_adopt_leaf(t, g, j, first + j);
            reop += search_leaf_reopened(s, g, first + j);
        }
        for (int j = 0; j < cnt; j++)
            for (int e = lane; e < d.nfix; e += 64) t.fix[(size_t)j * d.nfix + e] = ident[(first + j) * d.nfix + e];
        if (REBASE && !search_rebases(*t.state)) { // (the same in every lane; cnt == 0: the retain kept nothing of it)
            if (lane == 0) n = search_rebase_root(t);
            n = __shfl(n, 0);
            for (int e = lane; e < d.nfix; e += 64) t.fix[e] = SEARCH_ROOT_FIX;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) reop += __shfl_xor(reop, o);
        dropped = !REBASE && __any(dropped);
        for (int e = lane; e < d.nx; e += 64) s.x0[(size_t)k * d.nx + e] = g.x0_next[(size_t)k * d.nx + e];
        if (lane == 0) {
            search_adopt_scalars(s, t, k, n, !dropped);
            g.cover[k] = cnt;
            g.reopened[k] = reop;
        }
    }
}

// ---- rebase: retain<true> -> offsets<true> -> stage<true> -> rebase-rows -> adopt<true> (arithmetic: hmpc_search.h) -------------
// rebase-rows  one wavefront per staged leaf, grid-strided: the leaf's dual row crosses HBM once each way, verbatim, into row b of
//          the OTHER pool -- 16 bytes per lane and access where n_dual is even (every row then starts on a 16-byte boundary of
//          its pool), else 8 --, SEARCH_COPY_BATCH independent loads in flight before their stores, every output entry stored once;
//          lane 0 carries the bound: nx serial products against the row's lam_0, search_rebase_obj / search_rebase_bound.
//          No LDS, no workgroup barrier: a wave owns its row.  B: the staged leaves (<= row_cap; src[b] <= row_cap, the zero row).
#define SEARCH_COPY_BATCH 4
template <class V>
static __device__ __forceinline__ void search_copy_row(const V *__restrict__ in, V *__restrict__ out, const int n, const int lane)
{
    for (int j0 = 0; j0 < n; j0 += 64 * SEARCH_COPY_BATCH) {
        V v[SEARCH_COPY_BATCH];
#pragma unroll
        for (int u = 0; u < SEARCH_COPY_BATCH; u++) {
            const int j = j0 + u * 64 + lane;
            v[u] = in[j < n ? j : n - 1]; // (no predicate on the load: a lane beyond the end reads the last entry again and stores nothing)
        }
#pragma unroll
        for (int u = 0; u < SEARCH_COPY_BATCH; u++) {
            const int j = j0 + u * 64 + lane;
            if (j < n) out[j] = v[u];
        }
    }
}

__global__ void __launch_bounds__(64 * SEARCH_WAVES) hmpc_search_rebase_rows_kernel(const BranchDims d, const SearchState s, const SearchShift g, const int B,
                                                                                    double *__restrict__ q_dual, double *__restrict__ q_dual_obj)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nd = d.n_dual;
    for (long long w = (long long)blockIdx.x * SEARCH_WAVES + wave; w < B; w += (long long)gridDim.x * SEARCH_WAVES) {
        const size_t b = (size_t)w;
        const int32_t r = g.src[b];
        const double *in = s.p_dual + (size_t)r * nd;
        double *out = q_dual + b * nd;
        if ((nd & 1) == 0) search_copy_row((const double2 *)in, (double2 *)out, nd >> 1, lane);
        else search_copy_row(in, out, nd, lane);
        if (lane == 0) {
            const size_t k = (size_t)g.owner[b];
            const double obj = search_rebase_obj(in, s.p_dual_obj[r], g.x0_next + k * d.nx, s.x0 + k * d.nx, d.nx);
            uint8_t flag;
            g.lb_out[b] = search_rebase_bound(g.lb[b], obj, &flag);
            g.flags[b] = flag;
            q_dual_obj[b] = obj;
        }
    }
}

// ---- Host side: the entries of include/hmpc_search.h (arithmetic: hmpc_search.h) -----------------------------------------------
struct hmpc_search {
    hmpc_handle *h = nullptr;
    BranchDims d{};
    SearchState v{};       // views into the blocks below
    DevBuf<int8_t> fix, b_fix;
    DevBuf<double> lb, td, x0, p_obj, p_dual_obj, p_primal, p_dual, b_x0;
    DevBuf<int32_t> row, wrow, ti, p_status, p_iters, picks, count, offset, word, b_idx;
    DevBuf<uint8_t> alive;
    DevBuf<char> tmp;      // begin's compact trees, the outputs of results and leaves (hmpc_stage.h; exact fit, one blocking copy per array)
    PinBuf<int32_t> h_word;
    // hmpc_search_advance, allocated at its first call: the staging of SearchShift, the second dual pool, pinned mirrors
    SearchShift a{};
    DevBuf<int32_t> a_idx;
    DevBuf<int8_t> a_fix;
    DevBuf<uint8_t> a_flags;
    DevBuf<double> a_val, q_dual, q_dual_obj; // q_*: the pool the next shift writes (the two swap with every advance)
    PinBuf<double> a_hval;                    // e0 | x0_next on their way up
    PinBuf<int32_t> a_hidx;                   // word (4) | cover | reopened on their way down
    DevBuf<int32_t> srow, sleft, plev, pfirst; // speculation: the waiting records of the nodes, the blocks of the staged picks
    // anytime searches (include/hmpc_search_anytime.h): the trees a round found out of budget; the outputs of hmpc_search_bounds
    DevBuf<int32_t> open, bd_open;
    DevBuf<double> bd_val;                    // lower | upper
    PinBuf<int32_t> h_bd_open;
    PinBuf<double> h_bd_val;
    int32_t row0 = 0;      // first pool row of the staged (or next) round
    int32_t staged = 0;    // rows of the staged round (with waiting records a staged round may have none)
    int32_t staged_picks = 0, staged_waiting = 0; // its picks, 0: no round is staged / those of them whose record waits
    int64_t counters[4] = {0, 0, 0, 0}; // since begin: rounds consumed, QP launches, rows launched, picks served from waiting records
    bool begun = false;
};

// rows a round may stage at speculation depth `spec`: every pick a whole block, but never more than the pool holds
static size_t search_batch_rows(const hmpc_search *s, int spec)
{
    return std::min((size_t)s->v.K * SEARCH_MAX_WIDTH * (size_t)search_block_rows(spec), (size_t)s->v.row_cap);
}

// the staging of a round for `batch` rows (hmpc_search_create, hmpc_search_set_speculation: launch paths do not allocate)
static hipError_t search_alloc_batch(hmpc_search *s, size_t batch)
{
    hipError_t e;
    if ((e = s->b_fix.alloc(batch * s->d.nfix)) != hipSuccess) return e;
    if ((e = s->b_x0.alloc(batch * s->d.nx)) != hipSuccess) return e;
    if ((e = s->b_idx.alloc(3 * batch)) != hipSuccess) return e;
    int32_t *bi = s->b_idx;
    s->v.b_fix = s->b_fix;
    s->v.b_x0 = s->b_x0;
    s->v.b_warm = bi;
    s->v.b_tree = bi + batch;
    s->v.b_node = bi + 2 * batch;
    return hipSuccess;
}

static dim3 search_grid(long long waves)
{
    const long long need = (waves + SEARCH_WAVES - 1) / SEARCH_WAVES;
    return dim3((unsigned)(need < 1 ? 1 : need < SEARCH_MAX_GRID ? need : SEARCH_MAX_GRID));
}

extern "C" int hmpc_search_create(hmpc_handle *h, int32_t K, int32_t node_cap, int32_t row_cap, hmpc_search **out)
{
    g_err.clear();
    if (out) *out = nullptr;
    if (K <= 0 || node_cap <= 0 || row_cap <= 0) return fail(HMPC_EINVAL, "search: K, node_cap and row_cap must be positive");
    if (!h || !out) return fail(HMPC_EINVAL, "search: null handle or out");
    if (h->cert.nub <= 0) return fail(HMPC_EINVAL, "search: the problem has no binaries (nub == 0)");
    if ((long long)K * SEARCH_MAX_WIDTH >= (1ll << 31) || (long long)K * node_cap >= (1ll << 31))
        return fail(HMPC_EINVAL, "search: K too large (a round's picks and the slabs are indexed with int32)");
    HIPCHK(hipSetDevice(h->device));
    std::unique_ptr<hmpc_search> s(new hmpc_search);
    s->h = h;
    const BranchDims d = s->d = branch_dims_of(h);
    const size_t nodes = (size_t)K * node_cap, rows = (size_t)row_cap, k = (size_t)K;
    const size_t batch = std::min(k * SEARCH_MAX_WIDTH, rows); // (a round that does not fit the pool is not staged)
    HIPCHK(s->fix.alloc(nodes * d.nfix));
    HIPCHK(s->lb.alloc(nodes));
    HIPCHK(s->row.alloc(nodes));
    HIPCHK(s->wrow.alloc(nodes));
    HIPCHK(s->alive.alloc(nodes));
    HIPCHK(s->ti.alloc(6 * k));
    HIPCHK(s->td.alloc(2 * k));
    HIPCHK(s->x0.alloc(k * d.nx));
    HIPCHK(s->p_obj.alloc(rows));
    HIPCHK(s->p_dual_obj.alloc(rows + 1)); // (one row of zeros behind the pool, for the shift of a leaf that carries none: hmpc_search_advance)
    HIPCHK(s->p_status.alloc(rows));
    HIPCHK(s->p_iters.alloc(rows));
    HIPCHK(s->p_primal.alloc(rows * d.n_primal));
    HIPCHK(s->p_dual.alloc((rows + 1) * d.n_dual));
    HIPCHK(hipMemset(s->p_dual + rows * d.n_dual, 0, d.n_dual * sizeof(double)));
    HIPCHK(hipMemset(s->p_dual_obj + rows, 0, sizeof(double)));
    HIPCHK(s->picks.alloc(k * SEARCH_MAX_WIDTH));
    HIPCHK(s->count.alloc(k));
    HIPCHK(s->offset.alloc(k));
    HIPCHK(s->word.alloc(6));
    HIPCHK(s->h_word.alloc(6));
    HIPCHK(s->srow.alloc(nodes));
    HIPCHK(s->sleft.alloc(nodes));
    HIPCHK(s->plev.alloc(k * SEARCH_MAX_WIDTH));
    HIPCHK(s->pfirst.alloc(k * SEARCH_MAX_WIDTH));
    HIPCHK(s->open.alloc(k));
    HIPCHK(s->bd_open.alloc(k));
    HIPCHK(s->bd_val.alloc(2 * k));
    HIPCHK(s->h_bd_open.alloc(k));
    HIPCHK(s->h_bd_val.alloc(2 * k));
    HIPCHK(hipMemset(s->open, 0, k * sizeof(int32_t)));
    int32_t *ti = s->ti;
    double *td = s->td;
    s->v = SearchState{K, node_cap, row_cap, s->fix, s->lb, s->row, s->wrow, s->alive, ti, ti + k, ti + 2 * k, ti + 3 * k, ti + 4 * k, ti + 5 * k,
                       td, td + k, s->x0, s->p_obj, s->p_dual_obj, s->p_status, s->p_iters, s->p_primal, s->p_dual, s->picks, s->count, s->offset, s->word,
                       nullptr, nullptr, nullptr, nullptr, nullptr, s->srow, s->sleft, s->plev, s->pfirst, 0, HMPC_RULE_BEST_FIRST, 0, s->open};
    HIPCHK(search_alloc_batch(s.get(), batch));
    *out = s.release();
    return HMPC_OK;
}

extern "C" int hmpc_search_destroy(hmpc_search *s)
{
    g_err.clear();
    if (!s) return HMPC_OK;
    (void)hipSetDevice(s->h->device);
    (void)hipDeviceSynchronize();
    delete s;
    return HMPC_OK;
}

extern "C" int hmpc_search_begin(hmpc_search *s, const double *x0, const int32_t *count, const int8_t *fix, const double *lb, const double *dual,
                                 const double *dual_obj)
{
    g_err.clear();
    if (!s || !x0) return fail(HMPC_EINVAL, "search: null argument (the search and x0 are required)");
    const BranchDims &d = s->d;
    const size_t K = (size_t)s->v.K;
    std::vector<int32_t> off;
    size_t total = 0;
    if (count) {
        if (!fix || !lb) return fail(HMPC_EINVAL, "search: a cover needs fix and lb");
        if ((dual != nullptr) != (dual_obj != nullptr)) return fail(HMPC_EINVAL, "search: dual rows and dual objectives go together");
        off.assign(K + 1, 0);
        for (size_t k = 0; k < K; k++) {
            if (count[k] < 0 || count[k] > s->v.node_cap) return fail(HMPC_EINVAL, "search: a tree's cover does not fit its slab (node_cap)");
            total += (size_t)count[k];
            if (total > (size_t)s->v.row_cap && dual) return fail(HMPC_EINVAL, "search: the covers' rows do not fit the pool (row_cap)");
            off[k + 1] = (int32_t)total;
        }
    }
    HIPCHK(hipSetDevice(s->h->device));
    HIPCHK(hipDeviceSynchronize()); // (a step begins: nothing of the last one is in flight)
    HIPCHK(hipMemcpy(s->x0, x0, K * d.nx * sizeof(double), hipMemcpyHostToDevice));
    SearchBegin g{nullptr, nullptr, nullptr, 0};
    if (count) {
        const StageTable t = stage_search_begin(stage_dims(s->h), K, total, off.data(), fix, lb);
        HIPCHK(s->tmp.grow(t.total, t.total, nullptr));
        char *base = s->tmp;
        const int rc = stage_each_up(t, base, false);
        if (rc) return rc;
        if (total && dual) {
            HIPCHK(hipMemcpy(s->p_dual, dual, total * d.n_dual * sizeof(double), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(s->p_dual_obj, dual_obj, total * sizeof(double), hipMemcpyHostToDevice));
        }
        g = SearchBegin{t.at<int32_t>(SB_OFFSET, base), t.at<int8_t>(SB_FIX, base), t.at<double>(SB_LB, base), dual != nullptr}; // (an empty cover too)
    }
    hipLaunchKernelGGL(hmpc_search_begin_kernel, search_grid((long long)K), dim3(64 * SEARCH_WAVES), 0, nullptr, d, s->v, g);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));
    s->row0 = dual ? (int32_t)total : 0;
    s->staged = s->staged_picks = s->staged_waiting = 0;
    std::fill(s->counters, s->counters + 4, (int64_t)0);
    s->begun = true;
    return HMPC_OK;
}

extern "C" int hmpc_search_set_speculation(hmpc_search *s, int32_t depth)
{
    g_err.clear();
    if (depth < 0 || depth > SEARCH_MAX_SPEC) return fail(HMPC_EINVAL, "search: the speculation depth must lie in 0 .. 4");
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    if (s->staged_picks > 0) return fail(HMPC_EINVAL, "search: a round is staged (hmpc_search_consume comes first)");
    if ((long long)s->v.K * SEARCH_MAX_WIDTH * search_block_rows(depth) >= (1ll << 31))
        return fail(HMPC_EINVAL, "search: K too large for this depth (a round's rows are indexed with int32)");
    const size_t batch = search_batch_rows(s, depth);
    if (batch > s->b_idx.size() / 3) { // (a shallower depth keeps the larger staging)
        HIPCHK(hipSetDevice(s->h->device));
        HIPCHK(hipDeviceSynchronize()); // (nothing that reads the old staging is in flight)
        HIPCHK(search_alloc_batch(s, batch));
    }
    s->v.spec = depth;
    return HMPC_OK;
}

extern "C" int hmpc_search_select(hmpc_search *s, int32_t width, double tol, int32_t handdown, int32_t *B, void *stream)
{
    g_err.clear();
    if (width < 1 || width > SEARCH_MAX_WIDTH) return fail(HMPC_EINVAL, "search: width must lie in 1 .. 64");
    if (!s || !B) return fail(HMPC_EINVAL, "search: null argument (the search and B are required)");
    if (!s->begun) return fail(HMPC_EINVAL, "search: no step has begun (hmpc_search_begin)");
    HIPCHK(hipSetDevice(s->h->device));
    hipStream_t st = (hipStream_t)stream;
    const int hd = handdown != 0;
    s->staged = s->staged_picks = s->staged_waiting = 0;
    const long long slots = (long long)s->v.K * width, most = search_block_rows(s->v.spec);
    hipLaunchKernelGGL(hmpc_search_select_kernel, dim3(s->v.K), dim3(SEARCH_SELECT_THREADS), 0, st, s->d, s->v, (int)width, tol);
    HIPCHK(hipGetLastError());
    if (s->v.spec > 0) {
        hipLaunchKernelGGL(hmpc_search_blocks_kernel, search_grid(slots), dim3(64 * SEARCH_WAVES), 0, st, s->d, s->v, (int)width);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(hmpc_search_offsets_kernel, dim3(1), dim3(SEARCH_SCAN_CHUNK), 0, st, s->d, s->v, (int)s->row0, hd);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hmpc_search_stage_kernel, search_grid(slots * most), dim3(64 * SEARCH_WAVES), 0, st, s->d, s->v, (int)width, hd);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->h_word, s->word, 6 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int32_t *w = s->h_word;
    if (w[0] < 0 || (long long)w[0] > slots * most) return fail(HMPC_EDEVICE, "search: the device returned a round size outside [0, K width S(depth)]");
    if (w[4] < 0 || (long long)w[4] > slots || w[5] < 0 || w[5] > w[4]) return fail(HMPC_EDEVICE, "search: the device returned a number of picks outside [0, K width]");
    *B = w[0];
    if (!w[3]) return fail(HMPC_ETOOBIG, "search: the round's records do not fit the pool (row_cap)");
    s->staged = w[0];
    s->staged_picks = w[4];
    s->staged_waiting = w[5];
    return HMPC_OK;
}

extern "C" int hmpc_search_staged(const hmpc_search *s, int32_t *picks, int32_t *B)
{
    g_err.clear();
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    if (picks) *picks = s->staged_picks;
    if (B) *B = s->staged;
    return HMPC_OK;
}

extern "C" int hmpc_search_counters(const hmpc_search *s, int64_t *out)
{
    g_err.clear();
    if (!s || !out) return fail(HMPC_EINVAL, "search: null argument");
    std::copy(s->counters, s->counters + 4, out);
    return HMPC_OK;
}

extern "C" int hmpc_search_batch(const hmpc_search *s, const double **d_x0, const int8_t **d_fix, hmpc_warm *d_warm, hmpc_result *d_rows, int32_t *row0)
{
    g_err.clear();
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    const BranchDims &d = s->d;
    const SearchState &v = s->v;
    const size_t r = (size_t)s->row0;
    if (d_x0) *d_x0 = v.b_x0;
    if (d_fix) *d_fix = v.b_fix;
    if (d_warm) *d_warm = hmpc_warm{v.p_primal, v.p_dual, v.b_warm, v.row_cap};
    if (d_rows) *d_rows = hmpc_result{v.p_obj + r, v.p_dual_obj + r, v.p_status + r, v.p_iters + r, v.p_primal + r * d.n_primal, v.p_dual + r * d.n_dual};
    if (row0) *row0 = s->row0;
    return HMPC_OK;
}

extern "C" int hmpc_search_put_records(hmpc_search *s, int32_t B, const hmpc_result *rec)
{
    g_err.clear();
    if (!s || !rec) return fail(HMPC_EINVAL, "search: null argument");
    if (!rec->obj || !rec->status || !rec->iters) return fail(HMPC_EINVAL, "search: obj, status and iters of the records are required");
    if (s->staged <= 0 || B != s->staged) return fail(HMPC_EINVAL, "search: the records are not those of the staged round (its size is B of hmpc_search_select)");
    HIPCHK(hipSetDevice(s->h->device));
    const BranchDims &d = s->d;
    const size_t r = (size_t)s->row0, n = (size_t)B;
    HIPCHK(hipMemcpy(s->v.p_obj + r, rec->obj, n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->v.p_status + r, rec->status, n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->v.p_iters + r, rec->iters, n * sizeof(int32_t), hipMemcpyHostToDevice));
    if (rec->dual_obj) HIPCHK(hipMemcpy(s->v.p_dual_obj + r, rec->dual_obj, n * sizeof(double), hipMemcpyHostToDevice));
    if (rec->primal) HIPCHK(hipMemcpy(s->v.p_primal + r * d.n_primal, rec->primal, n * d.n_primal * sizeof(double), hipMemcpyHostToDevice));
    if (rec->dual) HIPCHK(hipMemcpy(s->v.p_dual + r * d.n_dual, rec->dual, n * d.n_dual * sizeof(double), hipMemcpyHostToDevice));
    return HMPC_OK;
}

extern "C" int hmpc_search_consume(hmpc_search *s, double tol, void *stream)
{
    g_err.clear();
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    if (s->staged_picks <= 0) return fail(HMPC_EINVAL, "search: no round is staged (hmpc_search_select)");
    HIPCHK(hipSetDevice(s->h->device));
    hipLaunchKernelGGL(hmpc_search_consume_kernel, search_grid((long long)s->v.K), dim3(64 * SEARCH_WAVES), 0, (hipStream_t)stream, s->d, s->v, (int)s->row0, tol);
    HIPCHK(hipGetLastError());
    s->counters[0]++;
    s->counters[1] += s->staged > 0;
    s->counters[2] += s->staged;
    s->counters[3] += s->staged_waiting;
    s->row0 += s->staged;
    s->staged = s->staged_picks = s->staged_waiting = 0;
    return HMPC_OK;
}

extern "C" int hmpc_search_run(hmpc_search *s, int32_t width, double tol, int32_t handdown, int32_t max_rounds, void *stream, int32_t *rounds, int64_t *launched)
{
    g_err.clear();
    if (rounds) *rounds = 0;
    if (launched) *launched = 0;
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    for (int32_t r = 0; max_rounds <= 0 || r < max_rounds; r++) {
        int32_t B = 0;
        int rc = hmpc_search_select(s, width, tol, handdown, &B, stream);
        if (rc) return rc;
        if (s->staged_picks == 0) break; // (no pick: every tree has stopped)
        if (B > 0) { // (else every pick's record waits: a round without a launch)
            const double *x0;
            const int8_t *fix;
            hmpc_warm warm;
            hmpc_result rows;
            hmpc_search_batch(s, &x0, &fix, &warm, &rows, nullptr);
            // (as the host-pointer solve does: the hand-down kernel only where a node of the round receives a record)
            if ((rc = hmpc_solve_batch_device(s->h, x0, s->d.nx, fix, B, s->h_word[2] ? &warm : nullptr, &rows, stream))) return rc;
        }
        if ((rc = hmpc_search_consume(s, tol, stream))) return rc;
        if (rounds) ++*rounds;
        if (launched) *launched += B;
    }
    return HMPC_OK;
}

extern "C" int hmpc_search_results(hmpc_search *s, double *cost, double *u0, double *x1, int8_t *binaries, int32_t *solves, int32_t *leaves, int32_t *state,
                                   int32_t *uncertified)
{
    g_err.clear();
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    if (!s->begun) return fail(HMPC_EINVAL, "search: no step has begun (hmpc_search_begin)");
    HIPCHK(hipSetDevice(s->h->device));
    const BranchDims &d = s->d;
    const size_t K = (size_t)s->v.K;
    const StageTable t = stage_search_results(stage_dims(s->h), K, cost, u0, x1, binaries, solves, leaves, state, uncertified);
    if (!t.total) return HMPC_OK;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(s->tmp.grow(t.total, t.total, nullptr));
    char *base = s->tmp;
    const SearchResults r{t.ptr<double>(SR_COST, base), t.ptr<double>(SR_U0, base), t.ptr<double>(SR_X1, base), t.ptr<int8_t>(SR_BINARIES, base),
                          t.ptr<int32_t>(SR_SOLVES, base), t.ptr<int32_t>(SR_LEAVES, base), t.ptr<int32_t>(SR_STATE, base), t.ptr<int32_t>(SR_UNCERTIFIED, base)};
    hipLaunchKernelGGL(hmpc_search_results_kernel, search_grid((long long)K), dim3(64 * SEARCH_WAVES), 0, nullptr, d, s->v, r);
    HIPCHK(hipGetLastError());
    return stage_each_down(t, base, false);
}

extern "C" int hmpc_search_leaves(hmpc_search *s, int32_t *n, int32_t *owner, int8_t *fix, double *lb, double *dual, double *dual_obj, uint8_t *has_dual)
{
    g_err.clear();
    if (!s || !n) return fail(HMPC_EINVAL, "search: null argument (the search and n are required)");
    if (*n < 0) return fail(HMPC_EINVAL, "search: negative capacity");
    const size_t K = (size_t)s->v.K;
    std::vector<int32_t> cnt(K), off(K);
    int rc = hmpc_search_results(s, nullptr, nullptr, nullptr, nullptr, nullptr, cnt.data(), nullptr, nullptr);
    if (rc) return rc;
    long long total = 0;
    for (size_t k = 0; k < K; k++) { off[k] = (int32_t)total; total += cnt[k]; }
    const int32_t cap = *n;
    if (total >= (1ll << 31)) return fail(HMPC_ETOOBIG, "search: more than 2^31 leaves");
    *n = (int32_t)total;
    if (total > cap) return fail(HMPC_ETOOBIG, "search: more leaves than the caller's arrays hold (their number is in n)");
    if (!total) return HMPC_OK;
    const BranchDims &d = s->d;
    const StageTable t = stage_search_leaves(stage_dims(s->h), K, (size_t)total, off.data(), owner, fix, lb, dual, dual_obj, has_dual);
    HIPCHK(s->tmp.grow(t.total, t.total, nullptr));
    char *base = s->tmp;
    if ((rc = stage_each_up(t, base, false))) return rc;
    const SearchLeaves o{t.ptr<int32_t>(SL_OFFSET, base), t.ptr<int32_t>(SL_OWNER, base), t.ptr<int8_t>(SL_FIX, base), t.ptr<double>(SL_LB, base),
                         t.ptr<double>(SL_DUAL, base), t.ptr<double>(SL_DOBJ, base), t.ptr<uint8_t>(SL_HAS_DUAL, base)};
    hipLaunchKernelGGL(hmpc_search_leaves_kernel, search_grid((long long)K), dim3(64 * SEARCH_WAVES), 0, nullptr, d, s->v, o);
    HIPCHK(hipGetLastError());
    return stage_each_down(t, base, false);
}

// The staging of an advance and the second dual pool (callers that never advance pay nothing).
static int search_advance_setup(hmpc_search *s, hipStream_t st)
{
    if (s->a.keep) return HMPC_OK;
    const BranchDims &d = s->d;
    const size_t K = (size_t)s->v.K, nodes = K * s->v.node_cap, rows = (size_t)s->v.row_cap;
    const size_t cap = std::min(nodes, rows); // staged leaves at most: more are refused at the readback
    HIPCHK(s->a_idx.alloc(nodes + 4 * K + 4 + 2 * cap));
    HIPCHK(s->a_fix.alloc(2 * cap * d.nfix));
    HIPCHK(s->a_flags.alloc(cap));
    HIPCHK(s->a_val.alloc(2 * cap + K * d.nu + 2 * K * d.nx));
    HIPCHK(s->q_dual.alloc((rows + 1) * d.n_dual));
    HIPCHK(s->q_dual_obj.alloc(rows + 1));
    HIPCHK(s->a_hval.alloc(2 * K * d.nx));
    HIPCHK(s->a_hidx.alloc(4 + 2 * K));
    HIPCHK(hipMemsetAsync(s->q_dual + rows * d.n_dual, 0, d.n_dual * sizeof(double), st)); // (its row of zeros, as hmpc_search_create)
    HIPCHK(hipMemsetAsync(s->q_dual_obj + rows, 0, sizeof(double), st));
    int32_t *i = s->a_idx;
    int8_t *f = s->a_fix;
    double *v = s->a_val;
    SearchShift &a = s->a;
    a.kept = i; a.first = i + K; a.cover = i + 2 * K; a.reopened = i + 3 * K; a.word = i + 4 * K;
    a.owner = i + 4 * K + 4; a.src = a.owner + cap;
    a.fix = f; a.fix_out = f + cap * d.nfix;
    a.lb = v; a.lb_out = v + cap; a.u0 = v + 2 * cap; a.e0 = a.u0 + K * d.nu; a.x0_next = a.e0 + K * d.nx;
    a.flags = s->a_flags;
    a.keep = a.src + cap; // (last: it says that all of this is in place)
    return HMPC_OK;
}

extern "C" int hmpc_search_advance(hmpc_search *s, const double *e0, const double *x0_next, int32_t *cover, int32_t *reopened, void *stream)
{
    g_err.clear();
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    if (!s->begun) return fail(HMPC_EINVAL, "search: no step has begun (hmpc_search_begin)");
    if (s->staged_picks > 0) return fail(HMPC_EINVAL, "search: a round is staged (hmpc_search_consume comes first)");
    if (!s->h->dp.shift_Mmu) return fail(HMPC_EINVAL, "search: hmpc_set_shift_maps has not been called");
    HIPCHK(hipSetDevice(s->h->device));
    hipStream_t st = (hipStream_t)stream;
    int rc = search_advance_setup(s, st);
    if (rc) return rc;
    const BranchDims &d = s->d;
    const SearchShift &a = s->a;
    const size_t K = (size_t)s->v.K, state = K * d.nx;
    // e0 and x0_next through the pinned block (the readback below is behind both copies: the block is free again when this returns)
    double *up = s->a_hval;
    if (e0) std::copy(e0, e0 + state, up);
    else std::fill(up, up + state, 0.0);
    HIPCHK(hipMemcpyAsync(a.e0, up, state * sizeof(double), hipMemcpyHostToDevice, st));
    if (x0_next) {
        std::copy(x0_next, x0_next + state, up + state);
        HIPCHK(hipMemcpyAsync(a.x0_next, up + state, state * sizeof(double), hipMemcpyHostToDevice, st));
    }
    const dim3 trees = search_grid((long long)K), waves(64 * SEARCH_WAVES);
    hipLaunchKernelGGL(hmpc_search_retain_kernel<false>, trees, waves, 0, st, d, s->v, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hmpc_search_advance_offsets_kernel<false>, dim3(1), dim3(SEARCH_SCAN_CHUNK), 0, st, s->v, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hmpc_search_advance_stage_kernel<false>, trees, waves, 0, st, d, s->v, a, (int)(x0_next != nullptr));
    HIPCHK(hipGetLastError());
    int32_t *down = s->a_hidx;
    HIPCHK(hipMemcpyAsync(down, a.word, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // the one synchronisation of a step: how many leaves the shift is launched for
    const int32_t B = down[0];
    if (B < 0 || (long long)B > (long long)K * s->v.node_cap) return fail(HMPC_EDEVICE, "search: the device returned a number of kept leaves outside [0, K node_cap]");
    if (down[1]) return fail(HMPC_EINVAL, "search: a tree is still running (its state is 0): the step has not ended");
    if (!down[2]) return fail(HMPC_ETOOBIG, "search: the kept leaves do not fit the pool (row_cap)");
    if (B > 0) {
        const ShiftArgs g{B, (int)K, a.owner, s->v.x0, a.u0, a.e0, a.fix, a.lb, s->v.p_dual, s->v.p_dual_obj, a.src,
                          a.fix_out, a.lb_out, s->q_dual, s->q_dual_obj, a.flags};
        if ((rc = hmpc_launch_shift(s->h, g, st))) return rc;
    }
    hipLaunchKernelGGL(hmpc_search_adopt_kernel<false>, trees, waves, 0, st, d, s->v, a);
    HIPCHK(hipGetLastError());
    // the pools swap: rows 0 .. B - 1 of the next step's pool are the shifted leaves'
    std::swap(s->p_dual, s->q_dual);
    std::swap(s->p_dual_obj, s->q_dual_obj);
    s->v.p_dual = s->p_dual;
    s->v.p_dual_obj = s->p_dual_obj;
    s->row0 = B;
    s->staged = s->staged_picks = s->staged_waiting = 0;
    if (cover || reopened) {
        HIPCHK(hipMemcpyAsync(down + 4, a.cover, 2 * K * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (cover) std::copy(down + 4, down + 4 + K, cover);
        if (reopened) std::copy(down + 4 + K, down + 4 + 2 * K, reopened);
    }
    return HMPC_OK;
}

extern "C" int hmpc_search_rebase(hmpc_search *s, const double *x0_new, int32_t *cover, int32_t *reopened, void *stream)
{
    g_err.clear();
    if (!s || !x0_new) return fail(HMPC_EINVAL, "search: null argument (the search and x0_new are required)");
    if (!s->begun) return fail(HMPC_EINVAL, "search: no step has begun (hmpc_search_begin)");
    if (s->staged_picks > 0) return fail(HMPC_EINVAL, "search: a round is staged (hmpc_search_consume comes first)");
    HIPCHK(hipSetDevice(s->h->device));
    hipStream_t st = (hipStream_t)stream;
    int rc = search_advance_setup(s, st);
    if (rc) return rc;
    const BranchDims &d = s->d;
    const SearchShift &a = s->a;
    const size_t K = (size_t)s->v.K, state = K * d.nx;
    // x0_new through the pinned block, where an advance's x0_next goes (the readback below is behind the copy)
    double *up = s->a_hval;
    up += state;
    std::copy(x0_new, x0_new + state, up);
    HIPCHK(hipMemcpyAsync(a.x0_next, up, state * sizeof(double), hipMemcpyHostToDevice, st));
    const dim3 trees = search_grid((long long)K), waves(64 * SEARCH_WAVES);
    hipLaunchKernelGGL(hmpc_search_retain_kernel<true>, trees, waves, 0, st, d, s->v, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hmpc_search_advance_offsets_kernel<true>, dim3(1), dim3(SEARCH_SCAN_CHUNK), 0, st, s->v, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hmpc_search_advance_stage_kernel<true>, trees, waves, 0, st, d, s->v, a, 1);
    HIPCHK(hipGetLastError());
    int32_t *down = s->a_hidx;
    HIPCHK(hipMemcpyAsync(down, a.word, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // the one synchronisation: how many rows are re-based, and whether they fit
    const int32_t B = down[0];
    if (B < 0 || (long long)B > (long long)K * s->v.node_cap) return fail(HMPC_EDEVICE, "search: the device returned a number of kept leaves outside [0, K node_cap]");
    if (!down[2]) return fail(HMPC_ETOOBIG, "search: the kept leaves do not fit the pool (row_cap)");
    if (B > 0) {
        hipLaunchKernelGGL(hmpc_search_rebase_rows_kernel, search_grid((long long)B), waves, 0, st, d, s->v, a, (int)B, (double *)s->q_dual, (double *)s->q_dual_obj);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(hmpc_search_adopt_kernel<true>, trees, waves, 0, st, d, s->v, a);
    HIPCHK(hipGetLastError());
    // the pools swap: rows 0 .. B - 1 of the pool from here on are the kept leaves', compact
    std::swap(s->p_dual, s->q_dual);
    std::swap(s->p_dual_obj, s->q_dual_obj);
    s->v.p_dual = s->p_dual;
    s->v.p_dual_obj = s->p_dual_obj;
    s->row0 = B;
    s->staged = s->staged_picks = s->staged_waiting = 0;
    std::fill(s->counters, s->counters + 4, (int64_t)0);
    if (cover || reopened) {
        HIPCHK(hipMemcpyAsync(down + 4, a.cover, 2 * K * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (cover) std::copy(down + 4, down + 4 + K, cover);
        if (reopened) std::copy(down + 4 + K, down + 4 + 2 * K, reopened);
    }
    return HMPC_OK;
}

// Host copies of the staged round, of one tree and of pool rows: for a caller that solves elsewhere, and for inspection.
extern "C" int hmpc_search_get_batch(hmpc_search *s, int32_t B, double *x0, int8_t *fix, int32_t *warm, int32_t *tree, int32_t *node)
{
    g_err.clear();
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    if (s->staged <= 0 || B != s->staged) return fail(HMPC_EINVAL, "search: no round of this size is staged");
    HIPCHK(hipSetDevice(s->h->device));
    const size_t n = (size_t)B;
    if (x0) HIPCHK(hipMemcpy(x0, s->v.b_x0, n * s->d.nx * sizeof(double), hipMemcpyDeviceToHost));
    if (fix) HIPCHK(hipMemcpy(fix, s->v.b_fix, n * s->d.nfix, hipMemcpyDeviceToHost));
    if (warm) HIPCHK(hipMemcpy(warm, s->v.b_warm, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (tree) HIPCHK(hipMemcpy(tree, s->v.b_tree, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (node) HIPCHK(hipMemcpy(node, s->v.b_node, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HMPC_OK;
}

extern "C" int hmpc_search_tree(hmpc_search *s, int32_t k, int32_t *scalars6, double *bounds2, int8_t *fix, double *lb, int32_t *row, int32_t *wrow, uint8_t *alive)
{
    g_err.clear();
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    if (k < 0 || k >= s->v.K) return fail(HMPC_EINVAL, "search: no such tree");
    HIPCHK(hipSetDevice(s->h->device));
    HIPCHK(hipDeviceSynchronize());
    const SearchState &v = s->v;
    const size_t o = (size_t)k * v.node_cap, n = (size_t)v.node_cap;
    if (scalars6) {
        const int32_t *src[6] = {v.n, v.inc, v.inc_row, v.solves, v.uncertified, v.state};
        for (int i = 0; i < 6; i++) HIPCHK(hipMemcpy(scalars6 + i, src[i] + k, sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    if (bounds2) {
        HIPCHK(hipMemcpy(bounds2, v.ub + k, sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(bounds2 + 1, v.unc_lb + k, sizeof(double), hipMemcpyDeviceToHost));
    }
    if (fix) HIPCHK(hipMemcpy(fix, v.fix + o * s->d.nfix, n * s->d.nfix, hipMemcpyDeviceToHost));
    if (lb) HIPCHK(hipMemcpy(lb, v.lb + o, n * sizeof(double), hipMemcpyDeviceToHost));
    if (row) HIPCHK(hipMemcpy(row, v.row + o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (wrow) HIPCHK(hipMemcpy(wrow, v.wrow + o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (alive) HIPCHK(hipMemcpy(alive, v.alive + o, n, hipMemcpyDeviceToHost));
    return HMPC_OK;
}

extern "C" int hmpc_search_tree_waiting(hmpc_search *s, int32_t k, int32_t *srow, int32_t *sleft)
{
    g_err.clear();
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    if (k < 0 || k >= s->v.K) return fail(HMPC_EINVAL, "search: no such tree");
    HIPCHK(hipSetDevice(s->h->device));
    HIPCHK(hipDeviceSynchronize());
    const size_t o = (size_t)k * s->v.node_cap, n = (size_t)s->v.node_cap;
    if (srow) HIPCHK(hipMemcpy(srow, s->v.srow + o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (sleft) HIPCHK(hipMemcpy(sleft, s->v.sleft + o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HMPC_OK;
}

extern "C" int hmpc_search_rows(hmpc_search *s, int32_t first, int32_t count, const hmpc_result *host, int32_t write)
{
    g_err.clear();
    if (!s || !host) return fail(HMPC_EINVAL, "search: null argument");
    if (first < 0 || count < 0 || (long long)first + count > s->v.row_cap) return fail(HMPC_EINVAL, "search: rows outside the pool");
    HIPCHK(hipSetDevice(s->h->device));
    HIPCHK(hipDeviceSynchronize());
    const BranchDims &d = s->d;
    const SearchState &v = s->v;
    const size_t r = (size_t)first, n = (size_t)count;
    auto move = [write](void *host, void *dev, size_t bytes) { // (the pool's own arrays: no block, no layout)
        if (!host || !bytes) return hipSuccess;
        return write ? hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice) : hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
    };
    HIPCHK(move(host->obj, v.p_obj + r, n * sizeof(double)));
    HIPCHK(move(host->dual_obj, v.p_dual_obj + r, n * sizeof(double)));
    HIPCHK(move(host->status, v.p_status + r, n * sizeof(int32_t)));
    HIPCHK(move(host->iters, v.p_iters + r, n * sizeof(int32_t)));
    HIPCHK(move(host->primal, v.p_primal + r * d.n_primal, n * d.n_primal * sizeof(double)));
    HIPCHK(move(host->dual, v.p_dual + r * d.n_dual, n * d.n_dual * sizeof(double)));
    return HMPC_OK;
}

// ---- anytime searches: the entries of include/hmpc_search_anytime.h (arithmetic: hmpc_search.h) ---------------------------------
extern "C" int hmpc_search_set_rule(hmpc_search *s, int32_t rule)
{
    g_err.clear();
    if (rule < HMPC_RULE_BEST_FIRST || rule > HMPC_RULE_DIVE_THEN_BEST) return fail(HMPC_EINVAL, "search: the rule must lie in 0 .. 3 (HMPC_RULE_*)");
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    if (s->staged_picks > 0) return fail(HMPC_EINVAL, "search: a round is staged (hmpc_search_consume comes first)");
    s->v.rule = rule;
    return HMPC_OK;
}

extern "C" int hmpc_search_set_budget(hmpc_search *s, int32_t max_solves, void *stream)
{
    g_err.clear();
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    if (s->staged_picks > 0) return fail(HMPC_EINVAL, "search: a round is staged (hmpc_search_consume comes first)");
    // (stored as max_solves + 1, 0: none; a tree never consumes 2^31 - 1 picks, so the largest budget is as good as none)
    s->v.budget1 = max_solves < 0 ? 0 : max_solves == INT32_MAX ? INT32_MAX : max_solves + 1;
    if (!s->begun) return HMPC_OK; // (no tree has a state yet: begin writes them all)
    HIPCHK(hipSetDevice(s->h->device));
    const int threads = 64 * SEARCH_WAVES;
    hipLaunchKernelGGL(hmpc_search_reopen_kernel, search_grid(((long long)s->v.K + 63) / 64), dim3(threads), 0, (hipStream_t)stream, s->v);
    HIPCHK(hipGetLastError());
    return HMPC_OK;
}

extern "C" int hmpc_search_bounds(hmpc_search *s, double tol, double *lower, double *upper, int32_t *open, void *stream)
{
    g_err.clear();
    if (!s) return fail(HMPC_EINVAL, "search: null search");
    if (!s->begun) return fail(HMPC_EINVAL, "search: no step has begun (hmpc_search_begin)");
    if (s->staged_picks > 0) return fail(HMPC_EINVAL, "search: a round is staged (hmpc_search_consume comes first)");
    if (!lower && !upper && !open) return HMPC_OK;
    HIPCHK(hipSetDevice(s->h->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t K = (size_t)s->v.K;
    double *val = s->bd_val, *h_val = s->h_bd_val;
    int32_t *h_open = s->h_bd_open;
    hipLaunchKernelGGL(hmpc_search_bounds_kernel, search_grid((long long)K), dim3(64 * SEARCH_WAVES), 0, st, s->d, s->v, tol, val, val + K, (int32_t *)s->bd_open);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_val, val, 2 * K * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_open, s->bd_open, K * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // the one synchronisation of the call
    if (lower) std::copy(h_val, h_val + K, lower);
    if (upper) std::copy(h_val + K, h_val + 2 * K, upper);
    if (open) std::copy(h_open, h_open + K, open);
    return HMPC_OK;
}
