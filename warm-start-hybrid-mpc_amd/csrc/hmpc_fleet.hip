// hmpc_fleet.hip -- K closed loops advanced in lockstep behind the C ABI (include/hmpc.h, hmpc_fleet_*).
//
// What it replaces: the loop body of the reference's closed-loop study (notebooks/cart_pole_with_walls/
// statistical_analysis.py:93-196; plot_trajectory.py:19-45) -- per MPC step one warm-started branch and bound
// (warm_start_hmpc/branch_and_bound.py:408-499 with the brancher of controller.py:395-429) and one construction
// of the next warm start (controller.py:431-564) -- for K independent loops at once.
//
// Why here and not in Python: at a few hundred trees the per-node bookkeeping of an interpreted driver costs more
// than the kernels (round 1: 2 k steps/s against 500 k QP/s of kernel capacity).  The split is
//   host (this file): tree topology and bounds -- identifiers, lower bounds, which dual row a node carries; candidate
//     selection, prune / incumbent / branch; a few kilobytes per tree;
//   device: every multiplier.  A solved node's dual row is written by the QP kernel straight into a row pool and never
//     leaves HBM; children reference their parent's row by index; the node shift (hmpc_shift.hip) reads the leaves'
//     rows through that index and writes the next step's pool.  Per round the host uploads the candidates'
//     identifiers and initial states (112 B per node) and downloads objective, status and the multipliers of the
//     binaries' bounds (1.3 KB per node) through pinned staging, on one stream -- or, with hmpc_fleet_digest, the digest
//     of the round that hmpc_branch.hip computes behind the QP kernel: one block of 48 B per node at T nub = 80.
// Semantics per tree are those of warm_start_hmpc_amd/batched.py (feedforward_many / construct_warm_start_many),
// against which tests/test_fleet.py checks it step by step.
// The host's share of a step is in hmpc_tree.h, free of HIP, where it runs under sanitizers (tests/host/tree_driver.cpp);
// this file owns the buffers and does the copies, launches and synchronisations between those phases.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <vector>

#include "hmpc_tree.h" // FleetTree and the host logic of a round, a step and a shift (host only, testable under sanitizers)

struct hmpc_fleet {
    hmpc_handle *h = nullptr;
    int K = 0;
    FleetDims dims{};
    std::vector<FleetTree> trees;
    hipStream_t stream = nullptr; // (destroyed after the buffers below are released: hmpc_fleet_destroy)
    DevBuf<double> pool[2], dobj[2]; // rows: dobj[s].size()
    DevBuf<double> ppool; // primal rows of the current step's solved nodes (same row index as pool[cur])
    size_t used = 0;
    int cur = 0;
    // per-round device buffers and their pinned host mirrors (fleet_ensure_round)
    DevBuf<int8_t> d_fix, d_fix_out;
    PinBuf<int8_t> h_fix;
    DevBuf<double> d_x0, d_obj, d_lb, d_lb_out;
    PinBuf<double> h_x0, h_obj, h_nu, h_lb;
    DevBuf<int32_t> d_status, d_iters, d_owner, d_src, d_widx;
    PinBuf<int32_t> h_status, h_iters, h_owner, h_src, h_widx;
    DevBuf<uint8_t> d_flags;
    PinBuf<uint8_t> h_flags;
    int handdown = 1; // parent -> child hand-down of active sets (hmpc_fleet_options)
    int digest = 0;   // a round's results come back as the digest of hmpc_branch.hip, one block per round (hmpc_fleet_digest)
    DevBuf<char> d_digest; // per node: obj, two child bounds, the words of rounded bits, word, pos -- array after array (fleet_digest_layout)
    PinBuf<char> h_digest;
    DevBuf<double> d_kx0, d_ku0, d_ke0; // K x nx, K x nu, K x nx
    PinBuf<double> h_k;                 //   their pinned mirror (3 blocks)
    PinBuf<double> h_bits;              // dive prediction: primal rows of a round's nodes
    PinBuf<double> h_prow;              // K primal rows: pinned / device (incumbents of a step)
    DevBuf<double> d_prow;
    PinBuf<int32_t> h_inc;              // K: pool row of each loop's incumbent
    DevBuf<int32_t> d_inc;
    long long rounds = 0, launched = 0, handed = 0;
    long long uncertified = 0, resting = 0; // nodes pruned without a certificate; searches whose optimum rests on such a prune (hmpc_fleet_uncertified)
    double t_select = 0, t_stage = 0, t_device = 0, t_consume = 0, t_shift = 0; // host wall time by phase (hmpc_fleet_timing)
    bool broken = false; // a call failed midway: the trees are half updated until hmpc_fleet_reset(f, -1)
};

// Rows `rows[k]` of a pool into a dense block (the incumbents' primal rows at the end of a step: one launch and one copy
// instead of one synchronous copy per new incumbent -- 1024 loops x ~17 us were a quarter of a step's wall time).
__global__ void hmpc_gather_rows(const double *__restrict__ pool, const int32_t *__restrict__ rows, int width, double *__restrict__ out)
{
    const int k = blockIdx.x, r = rows[k];
    if (r < 0) return;
    for (int j = threadIdx.x; j < width; j += blockDim.x) out[(size_t)k * width + j] = pool[(size_t)r * width + j];
}

namespace {

// An error in the middle of a step leaves some trees advanced and others not: the fleet refuses further steps until the
// caller has reset it (hmpc_fleet_reset(f, -1)).
int fleet_fail(hmpc_fleet *f, int code, const std::string &msg)
{
    f->broken = true;
    return fail(code, msg + " -- the fleet must be reset (hmpc_fleet_reset(f, -1)) before it is used again");
}

// A call that returns before it is done leaves the fleet broken.
struct BrokenUnlessDone {
    hmpc_fleet *f;
    bool ok = false;
    ~BrokenUnlessDone() { if (!ok) f->broken = true; }
};

// Host wall time by phase (hmpc_fleet_timing): from construction, or the last next(), to the next next() or the end of the
// scope goes to the slot named last.
struct Phase {
    double *slot;
    double t0 = now();
    explicit Phase(double &s) : slot(&s) {}
    Phase(const Phase &) = delete;
    ~Phase() { *slot += now() - t0; }
    void next(double &s)
    {
        const double t = now();
        *slot += t - t0;
        slot = &s;
        t0 = t;
    }
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
};

// The digest of a round of B nodes as ONE block, so that one copy brings it back: obj (B doubles) | child bounds (2 B doubles)
// | rounded bits (B x words) | word (B) | pos (B).
struct FleetDigest { size_t obj, lb2, bits, word, pos, bytes; };
inline size_t fleet_digest_node_bytes(size_t words) { return 3 * sizeof(double) + words * sizeof(uint64_t) + 2 * sizeof(int32_t); }
inline FleetDigest fleet_digest_layout(size_t B, size_t words)
{
    FleetDigest L;
    L.obj = 0;
    L.lb2 = L.obj + B * sizeof(double);
    L.bits = L.lb2 + 2 * B * sizeof(double);
    L.word = L.bits + B * words * sizeof(uint64_t);
    L.pos = L.word + B * sizeof(int32_t);
    L.bytes = L.pos + B * sizeof(int32_t);
    return L;
}

// Room in the round buffers for B nodes: one that is short is replaced by room for max(2B, 1024) nodes.
int fleet_ensure_round(hmpc_fleet *f, size_t B)
{
    const DevProb &p = f->h->dp;
    const size_t cap = std::max<size_t>(2 * B, 1024), nfix = (size_t)f->dims.nfix;
    hipError_t e = hipSuccess;
    auto grow = [&](auto &buf, size_t per_node) { if (e == hipSuccess) e = buf.grow(B * per_node, cap * per_node, f->stream); };
    grow(f->d_fix, nfix); grow(f->h_fix, nfix); grow(f->d_fix_out, nfix);
    grow(f->d_x0, p.nx); grow(f->h_x0, p.nx);
    grow(f->d_obj, 1); grow(f->h_obj, 1);
    grow(f->h_nu, 2 * nfix);
    grow(f->d_status, 1); grow(f->h_status, 1); grow(f->d_iters, 1); grow(f->h_iters, 1);
    grow(f->d_owner, 1); grow(f->h_owner, 1); grow(f->d_src, 1); grow(f->h_src, 1);
    grow(f->d_widx, 1); grow(f->h_widx, 1);
    grow(f->d_lb, 1); grow(f->h_lb, 1); grow(f->d_lb_out, 1);
    grow(f->d_flags, 1); grow(f->h_flags, 1);
    if (f->digest) { // (sized here with the other round buffers, never between the launches of a round)
        const size_t per = fleet_digest_node_bytes((nfix + 63) / 64);
        grow(f->d_digest, per); grow(f->h_digest, per);
    }
    if (e != hipSuccess) return fail(HMPC_EDEVICE, "fleet: cannot allocate the round buffers");
    return HMPC_OK;
}

// Room for `rows` rows in both pools (max(rows + rows / 2, 4096) where short); the rows in use of the current pool are kept.
int fleet_ensure_rows(hmpc_fleet *f, size_t rows)
{
    const DevProb &p = f->h->dp;
    const size_t cap = std::max<size_t>(rows + rows / 2, 4096);
    hipError_t e = hipSuccess;
    for (int s = 0; s < 2 && e == hipSuccess; s++) {
        const size_t keep = s == f->cur ? f->used : 0;
        e = f->pool[s].grow(rows * p.n_dual, cap * p.n_dual, f->stream, keep * p.n_dual);
        if (e == hipSuccess) e = f->dobj[s].grow(rows, cap, f->stream, keep);
    }
    if (e == hipSuccess) e = f->ppool.grow(rows * p.n_primal, cap * p.n_primal, f->stream, f->used * p.n_primal);
    if (e != hipSuccess) return fail(HMPC_EDEVICE, "fleet: cannot grow the row pools");
    return HMPC_OK;
}

} // namespace

extern "C" int hmpc_fleet_create(hmpc_handle *h, int32_t K, hmpc_fleet **out)
{
    g_err.clear();
    if (!h || !out || K < 1) return fail(HMPC_EINVAL, "fleet: null handle or K < 1");
    if (!h->dp.shift_Mmu) return fail(HMPC_EINVAL, "fleet: hmpc_set_shift_maps has not been called");
    HIPCHK(hipSetDevice(h->device));
    std::unique_ptr<hmpc_fleet> f(new hmpc_fleet());
    f->h = h;
    f->K = K;
    const DevProb &p = h->dp;
    f->dims = fleet_dims(p.nx, p.nu, p.nub, p.T, p.nc, p.ncL, p.nq, p.nr, p.nqT);
    if (f->dims.n_primal != p.n_primal || f->dims.n_dual != p.n_dual) return fail(HMPC_EINVAL, "fleet: the record sizes of hmpc_tree.h are not the handle's");
    f->trees.resize(K);
    for (auto &t : f->trees) {
        tree_reset_cold(t, f->dims.nfix);
        t.x0.assign(p.nx, 0.0);
    }
    const bool ok = f->d_kx0.alloc((size_t)K * p.nx) == hipSuccess && f->d_ku0.alloc((size_t)K * p.nu) == hipSuccess &&
                    f->d_ke0.alloc((size_t)K * p.nx) == hipSuccess && f->h_k.alloc((size_t)K * (2 * p.nx + p.nu)) == hipSuccess &&
                    f->h_prow.alloc((size_t)K * p.n_primal) == hipSuccess && f->d_prow.alloc((size_t)K * p.n_primal) == hipSuccess &&
                    f->h_inc.alloc((size_t)K) == hipSuccess && f->d_inc.alloc((size_t)K) == hipSuccess;
    if (!ok) return fail(HMPC_EDEVICE, "fleet: cannot allocate");
    // (the stream last: nothing else of the fleet is left to release if it cannot be created)
    if (hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess) return fail(HMPC_EDEVICE, "fleet: cannot create a stream");
    *out = f.release();
    return HMPC_OK;
}

extern "C" int hmpc_fleet_destroy(hmpc_fleet *f)
{
    if (!f) return HMPC_OK;
    (void)hipSetDevice(f->h->device);
    const hipStream_t stream = f->stream;
    if (stream) (void)hipStreamSynchronize(stream);
    delete f; // (releases every buffer)
    if (stream) (void)hipStreamDestroy(stream);
    return HMPC_OK;
}

extern "C" int hmpc_fleet_reset(hmpc_fleet *f, int32_t k)
{
    if (!f || k < -1 || k >= f->K) return fail(HMPC_EINVAL, "fleet: bad loop index");
    for (int i = (k < 0 ? 0 : k); i < (k < 0 ? f->K : k + 1); i++) tree_reset_cold(f->trees[i], f->dims.nfix);
    if (k < 0) f->broken = false;
    return HMPC_OK;
}

// Loop k has ended (its MIQP had no solution, or its caller has no further use for it): its tree is dropped and the loop
// takes no part in further steps -- no launches, no rows held in the pools -- until hmpc_fleet_reset makes it cold again.
extern "C" int hmpc_fleet_stop(hmpc_fleet *f, int32_t k)
{
    if (!f || k < 0 || k >= f->K) return fail(HMPC_EINVAL, "fleet: bad loop index");
    tree_reset_cold(f->trees[k], f->dims.nfix);
    f->trees[k].running = false;
    return HMPC_OK;
}

// Rows of the pools in use.  (For tests and reports: a fleet that is reset and solved at every step -- the cold searches
// of a closed-loop study -- must not grow with the number of steps.)
extern "C" int hmpc_fleet_rows(const hmpc_fleet *f, int64_t *used, int64_t *capacity)
{
    if (!f) return fail(HMPC_EINVAL, "fleet: null argument");
    if (used) *used = (int64_t)f->used;
    if (capacity) *capacity = (int64_t)f->dobj[0].size();
    return HMPC_OK;
}

// One MPC step of every running loop: branch and bound from the loop's current tree (the root for a cold loop).
// speculation = k > 0: with every candidate that has to be solved, its descendants through the next k binaries (2 + 4 +
// ... + 2^k nodes) ride in the same launch; their results wait in a per-tree cache and are consumed -- unchanged -- if and
// when the search selects them, so incumbent, leaves and solve counts are those of the search without speculation and only
// the number of launches drops (a warm-started step: from five to one or two).  Worth it for few loops (latency), a waste
// for many (throughput).
extern "C" int hmpc_fleet_solve(hmpc_fleet *f, const double *x0, int32_t width, int32_t speculation, double tol, double *cost,
                                double *u0, double *x1, int32_t *solves, int32_t *n_leaves)
{
    g_err.clear();
    if (!f || !x0) return fail(HMPC_EINVAL, "fleet: null argument");
    if (f->broken) return fail(HMPC_EINVAL, "fleet: an earlier call failed midway; reset the fleet (hmpc_fleet_reset(f, -1)) first");
    BrokenUnlessDone guard{f};
    if (width < 1) width = 1;
    // speculation < 0: DIVE PREDICTION (for few loops: it fetches the primal rows of every round).  A branch-and-bound dive
    // follows the relaxation: where a parent's relaxed binaries round to, its descendants' mostly stay.  With a picked node
    // whose parent's record is at hand, the whole predicted rest of the dive -- the node extended by the parent's rounded
    // binaries, one more at a time -- and the sibling of every step ride in the same launch: 2 (T nub - depth) nodes, linear
    // in the depth where the subtree expansion (speculation > 0) is exponential.  Results wait in the cache and are consumed
    // only if and when the search selects those nodes: incumbent, leaves and solve counts are those of the search without it.
    // A cold start is then the root, one launch with the predicted dive, and what the prediction missed.
    FleetExpansion ex{std::max(speculation, 0), speculation < 0, f->handdown != 0, {}, {}};
    hmpc_handle *h = f->h;
    HIPCHK(hipSetDevice(h->device));
    const FleetDims &d = f->dims;
    const int K = f->K, nfix = d.nfix, nx = d.nx;
    for (int k = 0; k < K; k++) tree_begin_step(f->trees[k], x0 + (size_t)k * nx, nx);
    if (fleet_pools_idle(f->trees)) f->used = 0;
    std::vector<std::vector<int>> picks(K);
    std::vector<FleetLaunch> launch;
    std::vector<int32_t> weak;
    for (;;) {
        // candidates of every tree: alive, bound below the incumbent; the `width` smallest bounds, first wins ties
        Phase phase(f->t_select);
        size_t npick = 0;
        for (int k = 0; k < K; k++) {
            tree_select(f->trees[k], width, tol, picks[k]);
            npick += picks[k].size();
        }
        if (npick == 0) break;
        // what has to be launched: picked nodes without a cached result, and what rides along with them
        phase.next(f->t_stage);
        const size_t B = fleet_count_round(f->trees, picks, d, ex);
        int rc, any_warm = 0;
        if (B > 0) {
            if ((rc = fleet_ensure_round(f, B))) return rc;
            if ((rc = fleet_ensure_rows(f, f->used + B))) return rc;
            any_warm = fleet_fill_round(f->trees, picks, d, ex, B, f->h_fix, f->h_x0, f->h_widx, launch);
            if (any_warm < 0) return fleet_fail(f, HMPC_EDEVICE, "fleet: the two passes over a round's nodes disagree on their number");
        }
        phase.next(B > 0 ? f->t_device : f->t_consume);
        if (B > 0) {
            HIPCHK(hipMemcpyAsync(f->d_fix, f->h_fix, B * nfix, hipMemcpyHostToDevice, f->stream));
            HIPCHK(hipMemcpyAsync(f->d_x0, f->h_x0, B * nx * sizeof(double), hipMemcpyHostToDevice, f->stream));
            double *rows = f->pool[f->cur] + f->used * d.n_dual;
            hmpc_result r{f->d_obj, f->dobj[f->cur] + f->used, f->d_status, f->d_iters, f->ppool + f->used * d.n_primal, rows};
            // (the parents' rows lie below f->used, this launch writes from f->used on)
            hmpc_warm hw{f->ppool, f->pool[f->cur], f->d_widx, (int32_t)f->used};
            if (any_warm) HIPCHK(hipMemcpyAsync(f->d_widx, f->h_widx, B * sizeof(int32_t), hipMemcpyHostToDevice, f->stream));
            if ((rc = hmpc_solve_batch_device(h, f->d_x0, nx, f->d_fix, (int32_t)B, any_warm ? &hw : nullptr, &r, f->stream))) return rc;
            if (f->digest) {
                // the digest kernel behind the QP kernel; one block comes back: 32 + 8 ceil(nfix / 64) bytes per node.  The cutoff
                // is decided on the host, at consumption (null here: +inf); the -inf of a weak node's dual objective is written there
                const size_t words = (size_t)(nfix + 63) / 64;
                const FleetDigest L = fleet_digest_layout(B, words);
                char *dd = f->d_digest, *hd = f->h_digest;
                hmpc_branch_out bo{};
                bo.obj = (double *)(dd + L.obj); bo.child_lb2 = (double *)(dd + L.lb2); bo.word = (int32_t *)(dd + L.word); bo.pos = (int32_t *)(dd + L.pos);
                if (ex.dive) bo.bits = (uint64_t *)(dd + L.bits);
                if ((rc = hmpc_branch_batch_device(h, f->d_fix, (int32_t)B, &r, nullptr, 0, 1, &bo, f->stream))) return rc;
                HIPCHK(hipMemcpyAsync(hd, dd, L.bytes, hipMemcpyDeviceToHost, f->stream));
                HIPCHK(hipStreamSynchronize(f->stream));
                phase.next(f->t_consume);
                f->rounds++;
                f->launched += (long long)B;
                const int handed = fleet_record_round_digest(f->trees, launch, d, (int32_t)f->used, B, f->h_fix, (const double *)(hd + L.obj), (const int32_t *)(hd + L.word),
                                                             (const int32_t *)(hd + L.pos), (const double *)(hd + L.lb2),
                                                             ex.dive ? (const uint64_t *)(hd + L.bits) : nullptr, words);
                if (handed < 0) return fleet_fail(f, HMPC_EDEVICE, "fleet: the digest's pos of a node is not the depth it was launched with");
                f->handed += handed;
                f->used += B;
            } else {
                HIPCHK(hipMemcpyAsync(f->h_obj, f->d_obj, B * sizeof(double), hipMemcpyDeviceToHost, f->stream));
                HIPCHK(hipMemcpyAsync(f->h_status, f->d_status, B * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
                HIPCHK(hipMemcpyAsync(f->h_iters, f->d_iters, B * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
                if (ex.dive) { // the round's primal rows: the rounded binaries of its vertex nodes predict their descendants' dives
                    if (f->h_bits.grow(B * d.n_primal, 2 * B * d.n_primal, f->stream) != hipSuccess)
                        return fail(HMPC_EDEVICE, "fleet: cannot allocate the prediction buffer");
                    HIPCHK(hipMemcpyAsync(f->h_bits, f->ppool + f->used * d.n_primal, B * d.n_primal * sizeof(double), hipMemcpyDeviceToHost, f->stream));
                }
                HIPCHK(hipMemcpy2DAsync(f->h_nu, 2 * nfix * sizeof(double), rows + d.o_lb, d.n_dual * sizeof(double), 2 * nfix * sizeof(double), B,
                                        hipMemcpyDeviceToHost, f->stream));
                HIPCHK(hipStreamSynchronize(f->stream));
                phase.next(f->t_consume);
                f->rounds++;
                f->launched += (long long)B;
                weak.clear();
                f->handed += fleet_record_round(f->trees, launch, d, (int32_t)f->used, B, f->h_fix, f->h_obj, f->h_status, f->h_iters, f->h_nu, 2 * (size_t)nfix,
                                                ex.dive ? (const double *)f->h_bits : nullptr, d.n_primal, weak);
                for (int32_t q : weak) { // (infeasible, but the ray is no proof to tolerance: the shift must reopen the leaf)
                    const double ninf = -std::numeric_limits<double>::infinity();
                    HIPCHK(hipMemcpy(f->dobj[f->cur] + f->used + q, &ninf, sizeof(double), hipMemcpyHostToDevice));
                }
                f->used += B;
            }
        }
        // prune / incumbent / branch, node by node in selection order (branch_and_bound.py:476-489)
        for (int k = 0; k < K; k++) {
            const int bad = tree_consume(f->trees[k], picks[k], nfix, tol);
            if (bad == 1) return fail(HMPC_EDEVICE, "fleet: a selected node has no result");
            if (bad == 2) return fleet_fail(f, HMPC_EDEVICE, "fleet: the QP solver did not converge on a node (status MAXITER / NUMERICAL)");
        }
    }
    // the incumbents' primal rows: one gather launch, one copy
    if (fleet_incumbent_rows(f->trees, f->h_inc)) {
        HIPCHK(hipMemcpyAsync(f->d_inc, f->h_inc, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice, f->stream));
        hipLaunchKernelGGL(hmpc_gather_rows, dim3(K), dim3(256), 0, f->stream, (const double *)f->ppool, (const int32_t *)f->d_inc, d.n_primal, f->d_prow);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(f->h_prow, f->d_prow, (size_t)K * d.n_primal * sizeof(double), hipMemcpyDeviceToHost, f->stream));
        HIPCHK(hipStreamSynchronize(f->stream));
    }
    // prunes without a certificate (HMPC_ITERS_UNCERTIFIED): counted; said aloud where a search's result rests on one
    const FleetUncertified unc = fleet_close_step(f->trees, d, f->h_inc, f->h_prow, cost, u0, x1, solves, n_leaves);
    if (unc.resting && !f->resting)
        fprintf(stderr, "hmpc: a branch-and-bound search pruned a node on the collapse of tau alone (no infeasibility certificate, HMPC_ITERS_UNCERTIFIED) "
                        "whose bound %.6g lay below the final incumbent %.6g: the returned optimum rests on that prune (hmpc_fleet_uncertified counts further ones)\n",
                unc.unc_lb, unc.ub);
    f->uncertified += unc.pruned;
    f->resting += unc.resting;
    guard.ok = true;
    return HMPC_OK;
}

// The next step's warm start of every running loop (controller.py:431-564): retain rule on the host (it only needs the
// identifiers and the applied binaries), everything that touches multipliers in one launch of the shift kernel.
extern "C" int hmpc_fleet_shift(hmpc_fleet *f, const double *e0, int32_t *cover, int32_t *reopened)
{
    g_err.clear();
    if (!f || !e0) return fail(HMPC_EINVAL, "fleet: null argument");
    if (f->broken) return fail(HMPC_EINVAL, "fleet: an earlier call failed midway; reset the fleet (hmpc_fleet_reset(f, -1)) first");
    BrokenUnlessDone guard{f};
    Phase phase(f->t_shift);
    hmpc_handle *h = f->h;
    HIPCHK(hipSetDevice(h->device));
    const FleetDims &d = f->dims;
    const int K = f->K, nx = d.nx, nu = d.nu;
    // kept leaves of all trees
    std::vector<std::vector<int>> keep(K);
    const size_t B = fleet_retain_leaves(f->trees, d, keep, cover, reopened);
    if (B == 0) { guard.ok = true; return HMPC_OK; }
    int rc = fleet_ensure_round(f, B);
    if (rc) return rc;
    if ((rc = fleet_ensure_rows(f, std::max(f->used, B)))) return rc;
    double *hx = f->h_k, *hu = hx + (size_t)K * nx, *he = hu + (size_t)K * nu;
    if (!fleet_stage_shift(f->trees, d, keep, e0, hx, hu, he, f->h_fix, f->h_owner, f->h_src, f->h_lb))
        return fail(HMPC_EINVAL, "fleet: a leaf carries no multipliers (unsolved root?)");
    HIPCHK(hipMemcpyAsync(f->d_kx0, hx, (size_t)K * nx * sizeof(double), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipMemcpyAsync(f->d_ku0, hu, (size_t)K * nu * sizeof(double), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipMemcpyAsync(f->d_ke0, he, (size_t)K * nx * sizeof(double), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipMemcpyAsync(f->d_fix, f->h_fix, B * d.nfix, hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipMemcpyAsync(f->d_owner, f->h_owner, B * sizeof(int32_t), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipMemcpyAsync(f->d_src, f->h_src, B * sizeof(int32_t), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipMemcpyAsync(f->d_lb, f->h_lb, B * sizeof(double), hipMemcpyHostToDevice, f->stream));
    const int nxt = f->cur ^ 1;
    ShiftArgs a{(int)B, K, f->d_owner, f->d_kx0, f->d_ku0, f->d_ke0, f->d_fix, f->d_lb, f->pool[f->cur], f->dobj[f->cur], f->d_src,
                f->d_fix_out, f->d_lb_out, f->pool[nxt], f->dobj[nxt], f->d_flags};
    if ((rc = hmpc_launch_shift(h, a, f->stream))) return rc;
    HIPCHK(hipMemcpyAsync(f->h_lb, f->d_lb_out, B * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    HIPCHK(hipMemcpyAsync(f->h_flags, f->d_flags, B, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));
    // the shifted leaves are the next tree: identifiers move one stage towards the present
    if (!fleet_adopt_shift(f->trees, d, keep, f->h_lb, f->h_flags, cover, reopened))
        return fail(HMPC_EDEVICE, "fleet: host and device disagree on the retain rule");
    f->cur = nxt;
    f->used = B;
    guard.ok = true;
    return HMPC_OK;
}

extern "C" int hmpc_fleet_uncertified(const hmpc_fleet *f, int64_t *pruned, int64_t *searches_resting_on_one)
{
    if (!f) return fail(HMPC_EINVAL, "fleet: null");
    if (pruned) *pruned = f->uncertified;
    if (searches_resting_on_one) *searches_resting_on_one = f->resting;
    return HMPC_OK;
}

extern "C" int hmpc_fleet_stats(const hmpc_fleet *f, int64_t *rounds, int64_t *launched)
{
    if (!f) return fail(HMPC_EINVAL, "fleet: null");
    if (rounds) *rounds = f->rounds;
    if (launched) *launched = f->launched;
    return HMPC_OK;
}

// Host wall time of the fleet's calls by phase since creation, seconds: candidate selection, staging of a round's nodes,
// device (copies, kernel, synchronisation), consumption of the results (prune / incumbent / branch), node shifts.
extern "C" int hmpc_fleet_timing(const hmpc_fleet *f, double *seconds5)
{
    if (!f || !seconds5) return fail(HMPC_EINVAL, "fleet: null");
    seconds5[0] = f->t_select; seconds5[1] = f->t_stage; seconds5[2] = f->t_device; seconds5[3] = f->t_consume; seconds5[4] = f->t_shift;
    return HMPC_OK;
}

// A round's results through the digest kernel (hmpc_branch.hip) and one copy, instead of three arrays, a strided copy of the
// multipliers' rows, the primal rows (dive prediction) and one blocking copy per weak node.  Off by default.
extern "C" int hmpc_fleet_digest(hmpc_fleet *f, int32_t enable)
{
    if (!f) return fail(HMPC_EINVAL, "fleet: null");
    if (enable >= 0) f->digest = enable != 0;
    return HMPC_OK;
}

extern "C" int hmpc_fleet_handdown(hmpc_fleet *f, int32_t enable, int64_t *verified)
{
    if (!f) return fail(HMPC_EINVAL, "fleet: null");
    if (enable >= 0) f->handdown = enable != 0;
    if (verified) *verified = f->handed;
    return HMPC_OK;
}
