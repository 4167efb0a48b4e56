// hmpc_capi.hip -- host side of the C ABI declared in include/hmpc.h.
//
// hmpc_create   : scales the stage constraints, builds the sparse row / column / Gram lists the
//                 kernel walks, uploads everything once (the role of controller.py:119-184, which
//                 builds the Gurobi model once per controller).
// hmpc_solve_*  : one kernel launch per batch of nodes (replaces B sequential calls of
//                 controller.py:229-271 + bounded_qp.py:200-228).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "hmpc_device.h"

#include "hmpc_kernel.hip" // one translation unit: the kernels are launched from this file
#include "hmpc_jit.h"      // register kernels for shapes without a built-in instantiation, compiled at hmpc_create
#include "hmpc_shift.hip"
#include "hmpc_certify.hip" // certificates of a batch of records (hmpc_certify_batch)
#include "hmpc_branch.hip"  // branching a batch of solved nodes (hmpc_branch_batch)
#include "hmpc_search.hip"  // the rounds of K device-resident searches (include/hmpc_search.h)

#define HMPC_CHECK_NODES 64 // (even) nodes of the first-use check of a kernel compiled at hmpc_create (hmpc_check_compiled)
static thread_local std::string g_err;
static int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
#define HIPCHK(call)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(HMPC_EDEVICE, std::string(#call) + ": " + hipGetErrorString(e_));        \
    } while (0)

// The one owner of device (hipMalloc) and pinned host (hipHostMalloc) memory in this library: a block of size() elements of
// T, released with its owner.  Converts to T * wherever a raw pointer is read (DevProb, kernel arguments, copies).
template <class T, bool Pinned>
class Buffer {
public:
    Buffer() = default;
    Buffer(Buffer &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buffer &operator=(Buffer &&o) noexcept
    {
        if (this != &o) { release(); std::swap(p_, o.p_); std::swap(n_, o.n_); }
        return *this;
    }
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    ~Buffer() { release(); }
    operator T *() const { return p_; }
    size_t size() const { return n_; }
    void release()
    {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    // a new block of n elements in place of the old one (at least one element is allocated: a view of an empty array is not null)
    hipError_t alloc(size_t n)
    {
        release();
        void *q = nullptr;
        const size_t bytes = (n ? n : 1) * sizeof(T);
        const hipError_t e = Pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
        if (e == hipSuccess) { p_ = (T *)q; n_ = n; }
        return e;
    }
    // Room for `want` elements: a block that is short (or absent) is replaced by one of `cap` elements -- the caller's slack --
    // once `stream` has finished with it; `keep` leading elements are copied across.
    hipError_t grow(size_t want, size_t cap, hipStream_t stream, size_t keep = 0)
    {
        if (p_ && want <= n_) return hipSuccess;
        hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;
        if (!p_ || !keep) return alloc(cap);
        Buffer next;
        if ((e = next.alloc(cap)) != hipSuccess) return e;
        if ((e = hipMemcpy(next.p_, p_, keep * sizeof(T), Pinned ? hipMemcpyHostToHost : hipMemcpyDeviceToDevice)) != hipSuccess) return e;
        *this = std::move(next);
        return hipSuccess;
    }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};
template <class T> using DevBuf = Buffer<T, false>;
template <class T> using PinBuf = Buffer<T, true>;

struct hmpc_cfg { // the kernel used for 1 / 2 / 4 waves per node, its LDS carve and resident-node count
    hmpc_kernel_choice k{};
    size_t lds = 0;
    int max_grid = 0;
    int sized = 0; // k is the run-time-sized kernel compiled with this problem's sizes (hmpc_jit_prepare_sized)
    int ilp = 0;   // ... with the compiler's ILP schedule: a binary the cache's VALIDATED manifest lists (hmpc_jit.h: sched_flags)
    // FIRST-USE CHECK of a kernel compiled at hmpc_create: `ref` is the shipped kernel that would serve this wave count without
    // the run-time compiler; the first launch through this configuration solves its first few nodes with both and compares
    // statuses and objectives (hmpc_check_compiled).  A kernel that disagrees is dropped for the handle.
    hmpc_kernel_choice ref{};
    size_t ref_lds = 0;
    int ref_grid = 0;
    int checked = 0; // 0 not yet, 1 agreed, -1 disagreed (ref serves)
    int second_opinions = 0; // batches with MAXITER / NUMERICAL nodes that the shipped kernel solved again and ended the same way (hmpc_solve_batch_device)
};

struct hmpc_handle {
    int device = 0;
    hmpc_cfg cfg[3];
    DevProb dp{};               // its pointers are views into the blocks below
    std::vector<DevBuf<char>> blocks;       // the problem's arrays (hmpc_create)
    std::vector<DevBuf<char>> shift_blocks; // the shift's maps (hmpc_set_shift_maps; a second call replaces them)
    const double *shift_MT2 = nullptr;      //   M_mu in pairs of columns, as hmpc_shift_row_kernel keeps it in LDS
    DevBuf<double> fac_ws;
    DevBuf<int> work_counter;
    DevBuf<double> rows_ws;
    DevBuf<int32_t> order; // processing order of large frontiers (hmpc_order_kernel)
    DevBuf<int32_t> pend;  // two-launch form of the lazy terminal set: [0] how many nodes wait for their second solve, [1 ..] which
    DevBuf<char> d_shift;  // staging of the host-pointer shift
    DevBuf<double> shift_tv; // per tree: what the shift needs of (x0, u0) only (hmpc_shift_tree_kernel)
    DevBuf<double> cert_mats; // the problem's UNSCALED matrices in one block, in the order of hmpc_problem (hmpc_certify_batch)
    CertProb cert{};          //   sizes, offsets of the rows and views into that block
    int cert_form = 0, cert_waves = 4, cert_per_cu = 4, cert_cus = 256; // form of hmpc_certify_kernel, chosen at hmpc_create (hmpc_certify_setup)
    size_t cert_lds = 0;
    DevBuf<double> trace;
    size_t lds = 0;
    int max_grid = 0, last_grid = 0;
    // staging for the host-pointer entry point
    DevBuf<char> d_stage; // one device block (inputs, then outputs: stage_layout)
    PinBuf<char> h_stage; // its pinned host mirror
    int last_cfg = -1;            // configuration (0, 1, 2: 1 / 2 / 4 waves per node) of the last launch
    // SECOND OPINION (hmpc_solve_batch_device): nodes a compiled kernel leaves undecided are listed on the device and solved again
    // by the shipped kernel in the same stream.  hard: [0] how many of them the shipped kernel leaves undecided too, [1] its work
    // counter, [2] how many the compiled kernel left, [3 ..] which.  The two counts of the last call travel to h_hard (pinned)
    // behind hard_done and are looked at when the next call comes, or when a caller that has synchronised asks (hmpc_second_opinion_review).
    DevBuf<int32_t> hard;
    PinBuf<int32_t> h_hard;
    hipEvent_t hard_done = nullptr;
    int hard_cfg = -1;            // configuration the counts in flight belong to (-1: none)
    int second_runs = 0;          // calls in which the shipped kernel was asked (for the tests)
    DevBuf<char> chk;             // device block of the first-use check (check_layout)
    PinBuf<char> h_chk;           //   its PINNED host mirror (objectives, dual objectives, statuses of the three runs, the hand-down index)
    int jit_rejected = 0;         //   compiled kernels dropped by it
    std::vector<void *> jit_libs; // shared objects of kernels compiled for this problem's shape (hmpc_jit.h); never unloaded
    int jit_kernels = 0;          //   how many of the three wave counts run on such a kernel (hmpc_kernel_info)
    hmpc_handle() = default;
    hmpc_handle(const hmpc_handle &) = delete;
    hmpc_handle &operator=(const hmpc_handle &) = delete;
    ~hmpc_handle() { if (hard_done) (void)hipEventDestroy(hard_done); }
};

namespace {

struct StageHost {
    int m, mg;
    std::vector<double> C, h, scale; // dense m x nz, scaled
    std::vector<int> rptr, rcol, cptr, crow, gptr, grow;
    std::vector<double> rval, cval, gval;
};

// [F G] rows scaled to unit norm, then the bound rows of the binaries.
void build_stage(const hmpc_problem &q, const double *F, const double *G, const double *h, int nrow, StageHost &s)
{
    const int nx = q.nx, nu = q.nu, nz = nx + nu, nub = q.nub, nuc = nu - nub;
    s.mg = nrow;
    s.m = nrow + 2 * nub;
    s.C.assign((size_t)s.m * nz, 0.0);
    s.h.assign(s.m, 0.0);
    s.scale.assign(nrow > 0 ? nrow : 1, 1.0);
    for (int r = 0; r < nrow; r++) {
        double n2 = 0;
        for (int j = 0; j < nx; j++) n2 += F[r * nx + j] * F[r * nx + j];
        for (int j = 0; j < nu; j++) n2 += G[r * nu + j] * G[r * nu + j];
        const double sc = n2 > 0 ? 1.0 / std::sqrt(n2) : 1.0;
        s.scale[r] = sc;
        for (int j = 0; j < nx; j++) s.C[(size_t)r * nz + j] = sc * F[r * nx + j];
        for (int j = 0; j < nu; j++) s.C[(size_t)r * nz + nx + j] = sc * G[r * nu + j];
        s.h[r] = sc * h[r];
    }
    for (int i = 0; i < nub; i++) {
        s.C[(size_t)(nrow + i) * nz + nx + nuc + i] = -1.0; // -ub <= 0
        s.C[(size_t)(nrow + nub + i) * nz + nx + nuc + i] = 1.0; // ub <= 1
        s.h[nrow + nub + i] = 1.0;
    }
    // rows
    s.rptr.assign(1, 0);
    for (int r = 0; r < s.m; r++) {
        for (int j = 0; j < nz; j++)
            if (s.C[(size_t)r * nz + j] != 0.0) { s.rcol.push_back(j); s.rval.push_back(s.C[(size_t)r * nz + j]); }
        s.rptr.push_back((int)s.rcol.size());
    }
    // columns
    s.cptr.assign(1, 0);
    for (int j = 0; j < nz; j++) {
        for (int r = 0; r < s.m; r++)
            if (s.C[(size_t)r * nz + j] != 0.0) { s.crow.push_back(r); s.cval.push_back(s.C[(size_t)r * nz + j]); }
        s.cptr.push_back((int)s.crow.size());
    }
    // Gram lists over the lower triangle, entry e = i (i + 1) / 2 + j
    s.gptr.assign(1, 0);
    for (int i = 0; i < nz; i++)
        for (int j = 0; j <= i; j++) {
            for (int r = 0; r < s.m; r++) {
                const double v = s.C[(size_t)r * nz + i] * s.C[(size_t)r * nz + j];
                if (v != 0.0) { s.grow.push_back(r); s.gval.push_back(v); }
            }
            s.gptr.push_back((int)s.grow.size());
        }
}

// Host arrays into blocks a handle owns, DevProb's pointers set to them.  After the first failure nothing more is uploaded:
// rc and hmpc_last_error hold that failure.
struct Uploader {
    std::vector<DevBuf<char>> &blocks;
    int rc = HMPC_OK;
    template <class T> void operator()(const std::vector<T> &v, const T *&view) { if (rc == HMPC_OK) rc = put(v, view); }
    template <class T> int put(const std::vector<T> &v, const T *&view)
    {
        DevBuf<char> d;
        HIPCHK(d.alloc((v.size() ? v.size() : 1) * sizeof(T)));
        if (!v.empty()) HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        view = (const T *)static_cast<char *>(d);
        blocks.push_back(std::move(d));
        return HMPC_OK;
    }
};

void upload_stage(Uploader &up, const StageHost &s, SparseStage &d)
{
    up(s.rptr, d.rptr); up(s.rcol, d.rcol); up(s.rval, d.rval);
    up(s.cptr, d.cptr); up(s.crow, d.crow); up(s.cval, d.cval);
    up(s.gptr, d.gptr); up(s.grow, d.grow); up(s.gval, d.gval);
    up(s.h, d.h); up(s.scale, d.scale);
}

// Wave counts for which this problem gets a register kernel compiled with its sizes (hmpc_jit_prepare_sized): placeholders
// (waves, kc) for hmpc_pick_kernel where the static row map holds the problem -- nx + nu <= 16, every [F G] row with
// at most two input coefficients, columns of at most HMPC_KC_STRIDE entries, at most 128 Gram entries with terms, at least one
// binary, at most 16 row slots per lane.  The two cart-pole shapes have built-in instantiations, which hmpc_pick_kernel finds
// itself; other problems leave jit empty and take the run-time-sized kernel.
void hmpc_jit_register_shapes(const DevProb &p, hmpc_kernel_choice (&jit)[3], size_t lds_cu)
{
    if (getenv("HMPC_FORCE_GENERIC") || getenv("HMPC_FORCE_BIG")) return;
    if ((p.nx == 4 && p.nu == 7 && p.nub == 4) || (p.nx == 4 && p.nu == 4 && p.nub == 2)) return; // (built in)
    if (!p.static_rows || p.nz > 16 || p.nub < 1) return;
    const int kc = std::max(2, (p.kcol + 1) / 2 * 2);
    if (kc > HMPC_KC_STRIDE || hmpc_lds_bytes(p, kc, 0) > lds_cu) return;
    for (int c = 0; c < 3; c++) {
        int kf = 0, kb = 0, kt = 0;
        if (!hmpc_static_slots(p, 1 << c, kf, kb, kt)) continue;
        if (kt < 1) kt = 1;                 // (the row map keeps a terminal slot; a problem without terminal set leaves it empty)
        if (kf + kb + kt > 16) continue;    // (row state in registers: 4 doubles per slot and lane)
        jit[c] = {(hmpc_kernel_t)(uintptr_t)1, (hmpc_kernel_t)(uintptr_t)1, 1 << c, kc, 0};
    }
}

// The integer sizes of a problem as assignments to the fields of DevProb: the body of HMPC_SIZED(p) of a kernel compiled for
// this problem alone (hmpc_jit.h), and with it the key of its cache entry.  Everything the kernels read as an int that is
// fixed once the problem is: dimensions, row counts and their splits, list lengths, the magic numbers of the divisions,
// the LDS choices of hmpc_create.  Tolerances, options and pointers stay arguments.
std::string hmpc_sized_fields(const DevProb &p)
{
    char b[1024];
    snprintf(b, sizeof b,
             "p.nx=%d;p.nu=%d;p.nub=%d;p.nuc=%d;p.nz=%d;p.T=%d;p.nc=%d;p.ncL=%d;p.nT=%d;p.mreg=%d;p.Toff=%d;p.M=%d;p.Mpad=%d;p.n=%d;p.ne=%d;"
             "p.nq=%d;p.nr=%d;p.nqT=%d;p.n_primal=%d;p.n_dual=%d;p.mreg_magic=%uu;p.nnz0=%d;p.nng0=%d;p.reg.m=%d;p.reg.mg=%d;p.kcol=%d;p.ngram=%d;"
             "p.ring=%d;p.nd=%d;p.ndp=%d;p.ns=%d;p.nd_magic=%uu;p.nn_magic=%uu;p.split_lds=%d;p.static_rows=%d;p.polish_l1=%d;",
             p.nx, p.nu, p.nub, p.nuc, p.nz, p.T, p.nc, p.ncL, p.nT, p.mreg, p.Toff, p.M, p.Mpad, p.n, p.ne, p.nq, p.nr, p.nqT, p.n_primal, p.n_dual,
             p.mreg_magic, p.nnz0, p.nng0, p.reg.m, p.reg.mg, p.kcol, p.ngram, p.ring, p.nd, p.ndp, p.ns, p.nd_magic, p.nn_magic, p.split_lds,
             p.static_rows, p.polish_l1);
    return b;
}

static bool hmpc_sized_enabled()
{
    if (getenv("HMPC_FORCE_GENERIC") || getenv("HMPC_FORCE_BIG")) return false; // (the run-time-sized kernels themselves are asked for)
    if (const char *e = getenv("HMPC_JIT")) { if (atoi(e) == 0) return false; }
    if (const char *e = getenv("HMPC_JIT_SIZED")) { if (atoi(e) == 0) return false; }
    return true;
}

// SIZED KERNELS (hmpc_jit.h): whatever kernel hmpc_pick_kernel chose for a wave count -- a register kernel of the problem's
// shape (built in, or a placeholder of hmpc_jit_prepare), the run-time-sized kernel or its streaming form -- is compiled with
// this problem's sizes as constants (or fetched from the cache) and replaces the choice in `cfg`.  Register kernels get
// exactly the row slots the horizon needs.  The streaming form runs four waves per node whatever the batch
// (hmpc_solve_batch_device), so only that one is built.  Returns false if a placeholder could not be replaced (the caller
// then falls back to the kernels without sizes).
bool hmpc_jit_prepare_sized(const DevProb &p, hmpc_cfg (&cfg)[3], std::vector<void *> &libs, int &count_out, std::vector<std::string> *built)
{
    const std::string fields = hmpc_sized_fields(p);
    hmpc_jit_shape shapes[3];
    int slot[3], count = 0;
    int only = -1;
    if (const char *e = getenv("HMPC_WAVES")) { const int nw = atoi(e); only = nw == 1 ? 0 : nw == 2 ? 1 : nw == 4 ? 2 : -1; }
    for (int c = 0; c < 3; c++) {
        const hmpc_kernel_choice &k = cfg[c].k;
        if (k.kc > 0) {                                                 // register kernel: the static row map with the slots this horizon needs
            int kf = 0, kb = 0, kt = 0;
            if (!hmpc_static_slots(p, k.waves, kf, kb, kt)) continue;
            if (kt < 1) kt = 1;
            shapes[count] = hmpc_jit_shape{p.nx, p.nu, p.nub, kf, kb, kt, k.waves, k.kc, fields};
            slot[count++] = c;
            continue;
        }
        if (k.big && c != (only >= 0 ? only : 2)) continue;
        // Row state (slack, multiplier, two steps per row) in registers instead of the global slab where a lane holds at most 16
        // rows (HMPC_JIT_SIZED_ROWS: another limit, 0: never): the list row map with Rows<Mpad / threads>.  configs[4], 12 rows
        // per lane: HBM traffic per launch 65 -> 45 GB, 137.0 -> 133.6 ms (profiles/r04_c4_rows_ab.txt); 164 B of scratch per lane.
        int rs = p.Mpad / (WAVE << c), rs_max = 16;
        if (const char *e = getenv("HMPC_JIT_SIZED_ROWS")) rs_max = atoi(e);
        if (rs > rs_max) rs = 0;
        shapes[count] = hmpc_jit_shape{k.big ? -1 : 0, -1, 0, rs, 0, 0, 1 << c, 0, fields};
        slot[count++] = c;
    }
    // the ILP schedule for the binaries the VALIDATED manifest lists (hmpc_jit.h: sched_flags), the default schedule for all others
    if (!getenv("HMPC_JIT_SCHED")) {
        const uint64_t hsh = hmpc_jit::source_hash();
        for (int i = 0; i < count; i++) {
            hmpc_jit_shape probe = shapes[i];
            probe.ilp = 1;
            if (hmpc_jit::validated(hmpc_jit::name_of(probe, hsh))) shapes[i].ilp = 1;
        }
    }
    std::vector<std::string> paths;
    std::string err;
    if (count) (void)hmpc_jit_build_all(shapes, count, paths, err);
    for (int i = 0; i < count; i++) {
        if (paths[i].empty()) continue;
        cfg[slot[i]].ilp = shapes[i].ilp || (getenv("HMPC_JIT_SCHED") && std::string(getenv("HMPC_JIT_SCHED")) != "default");
        if (built) {                                                     // (dry run: built, not loaded)
            bool seen = false;
            for (const std::string &b : *built) seen |= b == paths[i];
            if (!seen) built->push_back(paths[i]);
            cfg[slot[i]].sized = 1;
            continue;
        }
        void *lib = dlopen(paths[i].c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!lib) { err = std::string("dlopen: ") + dlerror(); continue; }
        auto get = (void (*)(void **, void **))dlsym(lib, "hmpc_jit_kernels");
        auto what = (const char *(*)(void))dlsym(lib, "hmpc_jit_sized");
        if (!get || !what || fields != what()) { err = "not the kernel of this problem: " + paths[i]; continue; } // (a collision of the key's hash)
        void *cold = nullptr, *warm = nullptr;
        get(&cold, &warm);
        libs.push_back(lib);
        cfg[slot[i]].k.fn = (hmpc_kernel_t)cold;
        cfg[slot[i]].k.fn_warm = (hmpc_kernel_t)warm;
        cfg[slot[i]].sized = 1;
        count_out++;
    }
    if (!err.empty() && getenv("HMPC_JIT_VERBOSE")) fprintf(stderr, "hmpc: sized kernel for this problem not available (%s): the kernel without sizes serves it\n", err.c_str());
    for (int c = 0; c < 3; c++)
        if (!cfg[c].sized && cfg[c].k.fn == (hmpc_kernel_t)(uintptr_t)1) return false;
    return true;
}

} // namespace

extern "C" const char *hmpc_last_error(void) { return g_err.c_str(); }

// Diagnostic (HMPC_BACKTRACE=1): the native frames of a fatal signal on stderr, then the default action.
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
static void hmpc_fatal_signal(int sig)
{
    void *frames[64];
    const int n = backtrace(frames, 64);
    static const char msg[] = "hmpc: fatal signal, native frames of the faulting thread:\n";
    (void)!write(2, msg, sizeof msg - 1);
    backtrace_symbols_fd(frames, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
static void hmpc_install_backtrace()
{
    static const bool once = [] {
        if (getenv("HMPC_BACKTRACE")) { signal(SIGSEGV, hmpc_fatal_signal); signal(SIGABRT, hmpc_fatal_signal); signal(SIGBUS, hmpc_fatal_signal); }
        return true;
    }();
    (void)once;
}

namespace {

constexpr size_t LDS_PER_CU = 160 * 1024;

// The host side of a problem (step (a) of hmpc_create): DevProb's sizes and options -- its pointers stay null -- and every array
// the kernels read except the caller's own, which setup_device uploads as they are.
struct HostProblem {
    DevProb p{};
    StageHost reg; // the stage rows; Gram lists in the order of ei / ej
    std::vector<double> ccv, Ct, ht, sct, P, PT, Cdn, sval;
    std::vector<int> cci, ei, ej, drow, rinfo, sptr, srow, nrow;
};

// dense / singleton split of the stage rows (generic kernel)
void split_rows(HostProblem &hp)
{
    DevProb &p = hp.p;
    const int nz = p.nz;
    const std::vector<double> &C = hp.reg.C;
    std::vector<int> &drow = hp.drow, &rinfo = hp.rinfo, &sptr = hp.sptr, &srow = hp.srow, &nrow = hp.nrow;
    std::vector<double> &sval = hp.sval, &Cdn = hp.Cdn;
    rinfo.assign(p.mreg, 0);
    sptr.assign(nz + 1, 0);
    sval.assign(p.mreg, 0.0);
    for (int r = 0; r < p.mreg; r++) {
        int cnt = 0, col = 0;
        for (int j = 0; j < nz; j++)
            if (C[(size_t)r * nz + j] != 0.0) { cnt++; col = j; }
        if (cnt >= 2) { rinfo[r] = -((int)drow.size() + 1); drow.push_back(r); }
        else { rinfo[r] = col; sval[r] = C[(size_t)r * nz + col]; }
    }
    p.nd = (int)drow.size();
    p.ndp = (p.nd + 3) / 4 * 4;
    Cdn.assign((size_t)p.ndp * nz, 0.0);
    for (int k = 0; k < p.nd; k++)
        for (int j = 0; j < nz; j++) Cdn[(size_t)k * nz + j] = C[(size_t)drow[k] * nz + j];
    drow.resize(p.ndp, 0);
    for (int j = 0; j < nz; j++) {
        for (int r = 0; r < p.mreg; r++)
            if (rinfo[r] == j && sval[r] != 0.0) srow.push_back(r);
        sptr[j + 1] = (int)srow.size();
    }
    p.ns = (int)srow.size();
    for (int r = 0; r < p.mreg; r++)
        if (rinfo[r] >= 0) nrow.push_back(r);
    p.nd_magic = p.nd > 0 ? (unsigned)((0x100000000ULL + p.nd - 1) / p.nd) : 0u;
    p.nn_magic = !nrow.empty() ? (unsigned)((0x100000000ULL + nrow.size() - 1) / nrow.size()) : 0u;
    if (nrow.empty()) nrow.push_back(0);
    if (Cdn.empty()) Cdn.push_back(0.0);
    if (drow.empty()) drow.push_back(0);
    if (srow.empty()) srow.push_back(0);
}

// (a) Validates the problem and builds its host side.  No HIP call.
int build_host_problem(const hmpc_problem &q, const hmpc_options *opt, HostProblem &hp)
{
    if (q.nx < 1 || q.nu < 1 || q.nub < 0 || q.nub > q.nu || q.T < 2 || q.nc < 0 || q.ncT < q.nc ||
        q.nq < 0 || q.nr < 0 || q.nqT < 0)
        return fail(HMPC_EINVAL, "inconsistent sizes (need nx,nu >= 1, 0 <= nub <= nu, T >= 2, ncT >= nc)");
    if (!q.A || !q.B || !q.F || !q.G || !q.h || !q.F_Tm1 || !q.G_Tm1 || !q.h_Tm1 || !q.Q || !q.R || !q.Q_T)
        return fail(HMPC_EINVAL, "null matrix pointer");
    DevProb &p = hp.p;
    StageHost &reg = hp.reg;
    const int nx = q.nx, nu = q.nu, nz = q.nx + q.nu;
    p.nx = q.nx; p.nu = q.nu; p.nub = q.nub; p.nuc = q.nu - q.nub; p.nz = q.nx + q.nu; p.T = q.T;
    p.nc = q.nc; p.ncL = q.ncT; p.nT = q.ncT - q.nc; p.mreg = q.nc + 2 * q.nub;
    p.Toff = q.T * p.mreg; p.M = p.Toff + p.nT; p.Mpad = (p.M + 255) / 256 * 256;
    p.n = q.T * p.nz + q.nx; p.ne = p.nz * (p.nz + 1) / 2;
    p.nq = q.nq; p.nr = q.nr; p.nqT = q.nqT;
    p.n_primal = (q.T + 1) * q.nx + q.T * q.nu;
    p.n_dual = (q.T + 1) * q.nx + (q.T - 1) * q.nc + q.ncT + 2 * q.T * q.nub + q.T * q.nq + q.nqT + q.T * q.nr;
    p.tol = opt && opt->tol > 0 ? opt->tol : 1e-8;
    p.tol_inf = opt && opt->tol_inf > 0 ? opt->tol_inf : 1e-6;
    p.max_iter = opt && opt->max_iter > 0 ? opt->max_iter : 100;
    p.lazy = opt ? opt->lazy_terminal : 1;
    p.refine = opt ? opt->refine : 1;
    p.dbg = getenv("HMPC_DBG") ? atoi(getenv("HMPC_DBG")) : 0;
    p.polish = opt ? opt->polish : 1;
    p.ptol = opt && opt->polish_tol > 0 ? opt->polish_tol : 1e-4;

    build_stage(q, q.F, q.G, q.h, q.nc, reg);
    p.reg.m = reg.m;
    p.reg.mg = reg.mg;
    p.mreg_magic = (unsigned)((0x100000000ULL + p.mreg - 1) / p.mreg);
    p.nnz0 = (int)reg.rcol.size();
    // columns of the stage rows padded to a fixed stride (compile-time shapes: static column products)
    hp.ccv.assign((size_t)nz * HMPC_KC_STRIDE, 0.0);
    hp.cci.assign((size_t)nz * HMPC_KC_STRIDE, 0);
    p.kcol = 0;
    for (int j = 0; j < nz; j++) {
        const int len = reg.cptr[j + 1] - reg.cptr[j];
        if (len > p.kcol) p.kcol = len;
        for (int k = 0; k < len && k < HMPC_KC_STRIDE; k++) {
            hp.ccv[(size_t)j * HMPC_KC_STRIDE + k] = reg.cval[reg.cptr[j] + k];
            hp.cci[(size_t)j * HMPC_KC_STRIDE + k] = reg.crow[reg.cptr[j] + k];
        }
    }
    p.static_rows = (p.kcol <= HMPC_KC_STRIDE && p.mreg <= 255) ? 1 : 0;
    for (int r = 0; r < q.nc; r++) {
        int cnt = 0;
        for (int j = 0; j < nu; j++) cnt += reg.C[(size_t)r * nz + nx + j] != 0.0;
        if (cnt > 2) p.static_rows = 0;
    }
    p.nng0 = (int)reg.grow.size();
    // The first nc rows of [F_Tm1 G_Tm1 | h_Tm1] must be the stage rows [F G | h] (controller.py:85-87):
    // the last stage then shares the stage lists and only the terminal-set rows are kept apart.
    for (int r = 0; r < q.nc; r++) {
        bool same = q.h_Tm1[r] == q.h[r];
        for (int j = 0; j < nx && same; j++) same = q.F_Tm1[r * nx + j] == q.F[r * nx + j];
        for (int j = 0; j < nu && same; j++) same = q.G_Tm1[r * nu + j] == q.G[r * nu + j];
        if (!same) return fail(HMPC_EINVAL, "the first nc rows of F_Tm1, G_Tm1, h_Tm1 must equal F, G, h");
    }
    // padded to a whole number of 256-row tiles (zero rows): a lane of the last row slot that has no terminal row
    // still addresses memory of these arrays
    const size_t nTpad = ((size_t)p.nT + 255) / 256 * 256 + 256;
    hp.Ct.assign(nTpad * nz, 0.0);
    hp.ht.assign(nTpad, 0.0);
    hp.sct.assign(nTpad, 1.0);
    for (int k = 0; k < p.nT; k++) {
        const int r = q.nc + k;
        double n2 = 0;
        for (int j = 0; j < nx; j++) n2 += q.F_Tm1[r * nx + j] * q.F_Tm1[r * nx + j];
        for (int j = 0; j < nu; j++) n2 += q.G_Tm1[r * nu + j] * q.G_Tm1[r * nu + j];
        const double sc = n2 > 0 ? 1.0 / std::sqrt(n2) : 1.0;
        hp.sct[k] = sc;
        for (int j = 0; j < nx; j++) hp.Ct[(size_t)k * nz + j] = sc * q.F_Tm1[r * nx + j];
        for (int j = 0; j < nu; j++) hp.Ct[(size_t)k * nz + nx + j] = sc * q.G_Tm1[r * nu + j];
        hp.ht[k] = sc * q.h_Tm1[r];
    }

    // cost Hessians, scaled so that their largest entry is one
    std::vector<double> &P = hp.P, &PT = hp.PT;
    P.assign((size_t)nz * nz, 0.0);
    PT.assign((size_t)nx * nx, 0.0);
    double big = 0;
    for (int i = 0; i < nx; i++)
        for (int j = 0; j < nx; j++) {
            double a = 0, b = 0;
            for (int k = 0; k < q.nq; k++) a += q.Q[k * nx + i] * q.Q[k * nx + j];
            for (int k = 0; k < q.nqT; k++) b += q.Q_T[k * nx + i] * q.Q_T[k * nx + j];
            P[(size_t)i * nz + j] = 2 * a;
            PT[(size_t)i * nx + j] = 2 * b;
            big = std::fmax(big, std::fmax(std::fabs(2 * a), std::fabs(2 * b)));
        }
    for (int i = 0; i < nu; i++)
        for (int j = 0; j < nu; j++) {
            double a = 0;
            for (int k = 0; k < q.nr; k++) a += q.R[k * nu + i] * q.R[k * nu + j];
            P[(size_t)(nx + i) * nz + nx + j] = 2 * a;
            big = std::fmax(big, std::fabs(2 * a));
        }
    p.cs = big > 0 ? 1.0 / big : 1.0;
    for (auto &v : P) v *= p.cs;
    for (auto &v : PT) v *= p.cs;
    {   // curvature of the (scaled) cost: smallest positive diagonal entry -- decides the penalty level of the polish (DevProb)
        double cmin = 1.0;
        for (int i = 0; i < nz; i++) if (P[(size_t)i * nz + i] > 0) cmin = std::fmin(cmin, P[(size_t)i * nz + i]);
        for (int i = 0; i < nx; i++) if (PT[(size_t)i * nx + i] > 0) cmin = std::fmin(cmin, PT[(size_t)i * nx + i]);
        p.polish_l1 = cmin >= 1e-2 ? 1 : 0;
    }

    // Number the entries with a nonempty Gram list first (the register factorisation gives one lane
    // to each of them); the lists follow the same numbering.
    {
        std::vector<int> ei, ej;
        for (int i = 0; i < nz; i++)
            for (int j = 0; j <= i; j++) { ei.push_back(i); ej.push_back(j); }
        std::vector<int> order;
        for (int pass = 0; pass < 2; pass++)
            for (int e = 0; e < p.ne; e++)
                if ((reg.gptr[e + 1] > reg.gptr[e]) == (pass == 0)) order.push_back(e);
        p.ngram = 0;
        for (int e = 0; e < p.ne; e++) p.ngram += reg.gptr[e + 1] > reg.gptr[e];
        std::vector<int> gptr2(1, 0), grow2;
        std::vector<double> gval2;
        for (int e : order) {
            hp.ei.push_back(ei[e]); hp.ej.push_back(ej[e]);
            for (int k = reg.gptr[e]; k < reg.gptr[e + 1]; k++) { grow2.push_back(reg.grow[k]); gval2.push_back(reg.gval[k]); }
            gptr2.push_back((int)grow2.size());
        }
        reg.gptr.swap(gptr2); reg.grow.swap(grow2); reg.gval.swap(gval2);
        if (p.ngram > 128) p.static_rows = 0; // (the shipped kernels take 64, hmpc_pick_kernel; kernels compiled for a shape two trips of 64)
    }
    split_rows(hp);
    if (p.M >= 65536 || p.mreg >= 65536) return fail(HMPC_ETOOBIG, "more than 65535 constraint rows per node");
    return HMPC_OK;
}

// (b) The kernel of each wave count (1 / 2 / 4 per node) with its LDS carve, and the LDS choices of the problem (DevProb:
// split_lds, ring).  With `built` (hmpc_jit_build_problem) the kernels compiled for this problem are built, not loaded.
int choose_kernels(DevProb &p, int lds_max, hmpc_cfg (&cfg)[3], std::vector<void *> &libs, int &jit_kernels, std::vector<std::string> *built)
{
    // generic kernel on the matrix cores (nz >= 16): the dense stage rows go to LDS if they fit beside everything else
    p.split_lds = 0;
    p.ring = 1;
    if (p.nz >= 16) {
        const bool big = hmpc_lds_bytes(p, 0, 0) > LDS_PER_CU || getenv("HMPC_FORCE_BIG");
        p.split_lds = 1;
        if (hmpc_lds_bytes(p, 0, big ? 1 : 0) > LDS_PER_CU) p.split_lds = 0;
    }
    // streaming form: as many stages per chunk of staged multipliers as LDS has room for
    for (int r = 2; r >= 1; r--) { // (two stages per chunk hide the slab latency: the barrier of a chunk costs 0.5 % of a solve)
        p.ring = r;
        if (hmpc_lds_bytes(p, 0, 1) <= LDS_PER_CU) break;
    }
    if (const char *e = getenv("HMPC_RING")) {
        const int r = atoi(e);
        if (r >= 1 && r <= 2) p.ring = r;
    }
    // shapes without a built-in instantiation: the register kernel is compiled now (or found in the cache), hmpc_jit.h
    hmpc_kernel_choice jit[3] = {};
    for (int pass = 0; pass < 2; pass++) {
        // first the kernels compiled with this problem's sizes (hmpc_jit.h); without them (HMPC_JIT_SIZED=0 / HMPC_JIT=0, no
        // compiler at run time, a compilation that fails) the shipped kernels: the built-in register kernels of the two
        // cart-pole shapes, the run-time-sized kernel for every other system
        const bool sized = pass == 0 && hmpc_sized_enabled();
        if (pass == 0 && !sized) continue;
        for (int c = 0; c < 3; c++) { jit[c] = hmpc_kernel_choice{}; cfg[c] = hmpc_cfg{}; }
        jit_kernels = 0; // (kernels of a first pass that did not complete are not in use)
        if (sized) hmpc_jit_register_shapes(p, jit, LDS_PER_CU);
        for (int c = 0; c < 3; c++) {
            hmpc_cfg &cf = cfg[c];
            cf.k = hmpc_pick_kernel(p, 1 << c, jit);
            cf.lds = hmpc_lds_bytes(p, cf.k.kc, cf.k.big);
            if (cf.lds > LDS_PER_CU || (lds_max > 0 && cf.lds > (size_t)lds_max)) {
                char msg[256];
                snprintf(msg, sizeof msg, "problem needs %zu bytes of LDS per node, more than one CU has (%d)", cf.lds, lds_max > 0 ? lds_max : (int)LDS_PER_CU);
                return fail(HMPC_ETOOBIG, msg);
            }
        }
        if (!sized || hmpc_jit_prepare_sized(p, cfg, libs, jit_kernels, built)) break;
    }
    return HMPC_OK;
}

// Resident nodes of a kernel with `lds` bytes of LDS per node: as many per CU as LDS admits, at most 8 (HMPC_BLOCKS_PER_CU: another number)
int resident_grid(size_t lds, int cus, const char *per_cu_env)
{
    int per_cu = (int)(LDS_PER_CU / lds);
    if (per_cu > 8) per_cu = 8;
    if (per_cu_env && atoi(per_cu_env) > 0) per_cu = atoi(per_cu_env);
    return (cus > 0 ? cus : 256) * per_cu;
}

// The first-use check's device block (hmpc_check_compiled): objectives, dual objectives, statuses and iterations of
// HMPC_CHECK_NODES nodes for each of its three runs, the hand-down index, the records of the compiled kernel's cold run and the
// check's own nodes -- initial states and fixing vectors (hmpc_check_set_kernel).  Its pinned host mirror has the same layout
// up to the records (`mirror` bytes).
struct CheckLayout {
    size_t obj, dobj, status, iters, idx, primal, dual, x0, fix, mirror, total;
};
CheckLayout check_layout(const DevProb &p)
{
    constexpr size_t N = HMPC_CHECK_NODES;
    static_assert(N % 2 == 0, "the records follow N int32 indices: N even keeps them 8-byte aligned");
    CheckLayout L;
    L.obj = 0;
    L.dobj = L.obj + 3 * N * sizeof(double);
    L.status = L.dobj + 3 * N * sizeof(double);
    L.iters = L.status + 3 * N * sizeof(int32_t);
    L.idx = L.iters + 3 * N * sizeof(int32_t);
    L.primal = L.idx + N * sizeof(int32_t);
    L.mirror = L.primal;
    L.dual = L.primal + N * p.n_primal * sizeof(double);
    L.x0 = L.dual + N * p.n_dual * sizeof(double);
    L.fix = L.x0 + N * p.nx * sizeof(double);
    L.total = L.fix + N * p.T * p.nub + 64;
    return L;
}

// (c) The device side of a handle whose kernels are chosen: the problem's arrays; the LDS of every kernel (a compiled kernel
// this device does not take gives way to the shipped one); the shipped kernels the first-use check compares against; the
// blocks of the check and of the second opinion; the workspaces.
int setup_device(hmpc_handle *h, const HostProblem &hp, const hmpc_problem &q, int cus, int lds_max)
{
    DevProb &p = h->dp;
    const int nx = q.nx, nu = q.nu;
    auto vec = [](const double *a, size_t n) { return std::vector<double>(a, a + n); };
    Uploader up{h->blocks};
    upload_stage(up, hp.reg, p.reg);
    up(hp.reg.C, p.Creg);
    up(hp.nrow, p.nrow); up(hp.Cdn, p.Cdn); up(hp.drow, p.drow); up(hp.rinfo, p.rinfo); up(hp.sval, p.sval); up(hp.sptr, p.sptr); up(hp.srow, p.srow);
    up(hp.ccv, p.ccv); up(hp.cci, p.cci);
    up(vec(q.F, (size_t)q.nc * nx), p.F_raw); up(vec(q.G, (size_t)q.nc * nu), p.G_raw); up(vec(q.h, (size_t)q.nc), p.h_raw);
    up(vec(q.h_Tm1, (size_t)q.ncT), p.hT_raw);
    up(hp.Ct, p.Ct); up(hp.ht, p.ht); up(hp.sct, p.sct);
    up(vec(q.A, (size_t)nx * nx), p.A); up(vec(q.B, (size_t)nx * nu), p.B); up(hp.P, p.P); up(hp.PT, p.PT);
    up(vec(q.Q, (size_t)q.nq * nx), p.Q); up(vec(q.R, (size_t)q.nr * nu), p.R); up(vec(q.Q_T, (size_t)q.nqT * nx), p.QT);
    up(hp.ei, p.ei); up(hp.ej, p.ej);
    if (up.rc) return up.rc;
    {   // the problem as the caller stated it, for the certificates: with this copy hmpc_certify_batch_device allocates nothing
        CertProb &c = h->cert;
        cert_set_sizes(c, q.nx, q.nu, q.nub, q.T, q.nc, q.ncT, q.nq, q.nr, q.nqT);
        std::vector<double> m;
        auto add = [&m](const double *a, size_t n) { m.insert(m.end(), a, a + n); };
        add(q.A, (size_t)nx * nx); add(q.B, (size_t)nx * nu);
        add(q.F, (size_t)q.nc * nx); add(q.G, (size_t)q.nc * nu); add(q.h, (size_t)q.nc);
        add(q.F_Tm1, (size_t)q.ncT * nx); add(q.G_Tm1, (size_t)q.ncT * nu); add(q.h_Tm1, (size_t)q.ncT);
        add(q.Q, (size_t)q.nq * nx); add(q.R, (size_t)q.nr * nu); add(q.Q_T, (size_t)q.nqT * nx);
        if (m.size() != cert_matrix_doubles(c) || c.n_dual != p.n_dual || c.n_primal != p.n_primal)
            return fail(HMPC_EINVAL, "the certificate's layout disagrees with the solver's");
        if (h->cert_mats.alloc(m.size()) != hipSuccess) return fail(HMPC_EDEVICE, "cannot allocate the certificate's matrices");
        HIPCHK(hipMemcpy(h->cert_mats, m.data(), m.size() * sizeof(double), hipMemcpyHostToDevice));
        cert_set_matrices(c, h->cert_mats);
    }

    const char *per_cu_env = getenv("HMPC_BLOCKS_PER_CU");
    auto fits = [&](size_t lds) { return lds <= LDS_PER_CU && (lds_max <= 0 || lds <= (size_t)lds_max); };
    auto reserve = [](const hmpc_cfg &f) {
        return hipFuncSetAttribute((const void *)f.k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds) == hipSuccess &&
               hipFuncSetAttribute((const void *)f.k.fn_warm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds) == hipSuccess;
    };
    for (int c = 0; c < 3; c++) {
        hmpc_cfg &cf = h->cfg[c];
        if (!reserve(cf)) {
            // a kernel from the cache that this device does not take (a stale or foreign object: another architecture, another
            // runtime): the shipped kernel of the wave count serves instead, as after a failed first-use check
            const hmpc_kernel_choice ship = hmpc_pick_kernel(p, 1 << c, nullptr);
            bool ok = false;
            if (ship.fn != cf.k.fn) {
                (void)hipGetLastError();
                if (getenv("HMPC_JIT_VERBOSE")) fprintf(stderr, "hmpc: the kernel compiled for this problem (%d waves per node) cannot be set up on this device: the shipped kernel serves\n", cf.k.waves);
                cf.k = ship;
                cf.lds = hmpc_lds_bytes(p, ship.kc, ship.big);
                cf.sized = 0;
                cf.ilp = 0;
                h->jit_rejected++;
                ok = fits(cf.lds) && reserve(cf);
            }
            if (!ok) return fail(HMPC_EDEVICE, "cannot reserve dynamic LDS for the kernel");
        }
        cf.max_grid = resident_grid(cf.lds, cus, per_cu_env);
        if (cf.max_grid > h->max_grid) h->max_grid = cf.max_grid;
    }
    h->lds = h->cfg[0].lds;
    // kernels compiled at hmpc_create are checked against the shipped kernel of the same wave count at their first launch
    const char *e = getenv("HMPC_JIT_SELFCHECK");
    const bool check = !(e && atoi(e) == 0);
    bool ref_big = false, any_ref = false;
    for (int c = 0; c < 3 && check; c++) {
        hmpc_cfg &cf = h->cfg[c];
        const hmpc_kernel_choice ref = hmpc_pick_kernel(p, 1 << c, nullptr);
        if (ref.fn == cf.k.fn) continue;                            // (a shipped kernel serves: nothing was compiled)
        const size_t lds = hmpc_lds_bytes(p, ref.kc, ref.big);
        if (!fits(lds)) continue;
        if (hipFuncSetAttribute((const void *)ref.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) continue;
        if (ref.fn_warm && hipFuncSetAttribute((const void *)ref.fn_warm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError(); // (its list mode is the second opinion's launch: without it that net is off for this wave count)
            continue;
        }
        cf.ref = ref;
        cf.ref_lds = lds;
        cf.ref_grid = resident_grid(lds, cus, nullptr);
        if (cf.ref_grid > h->max_grid) h->max_grid = cf.ref_grid;   // (the workspaces below must hold its launches too)
        ref_big = ref_big || ref.big;
        any_ref = true;
    }
    const CheckLayout L = check_layout(p);
    if (h->chk.alloc(L.total) != hipSuccess) return fail(HMPC_EDEVICE, "cannot allocate the check block");
    // (pinned: an asynchronous copy to or from pageable memory -- the stack arrays this check used until round 5 -- has the
    // runtime register the pages for its duration, and that bookkeeping did not survive eight host threads checking their
    // handles at once: heap corruption inside the runtime, one crash in ~30 calls of fleet.closed_loop_parallel with 8 fleets,
    // none in 180 with the check off; profiles/r05_fleet_trace.txt)
    if (h->h_chk.alloc(L.mirror) != hipSuccess) return fail(HMPC_EDEVICE, "cannot allocate the check block's host mirror");
    // second opinion of hmpc_solve_batch_device: its counts travel to two pinned words behind an event
    if (any_ref && (h->h_hard.alloc(2) != hipSuccess || hipEventCreateWithFlags(&h->hard_done, hipEventDisableTiming) != hipSuccess))
        return fail(HMPC_EDEVICE, "cannot allocate the second-opinion block");
    p.fac_ws = nullptr;
    p.fac_stride = 0;
    if (h->cfg[0].k.big || h->cfg[1].k.big || h->cfg[2].k.big || ref_big) {
        p.fac_stride = p.T * (p.nx * p.nu + p.nu * (p.nu - 1) / 2) + (p.T + 1) * (p.nx * (p.nx + 1) / 2);
        if (h->fac_ws.alloc((size_t)h->max_grid * p.fac_stride) != hipSuccess) return fail(HMPC_EDEVICE, "cannot allocate the factor workspace");
        p.fac_ws = h->fac_ws;
    }
    if (h->work_counter.alloc(2) != hipSuccess) return fail(HMPC_EDEVICE, "cannot allocate the work counter");
    p.work_counter = h->work_counter;
    (void)hipMemset(p.work_counter, 0, 2 * sizeof(int));
    p.check_flag = (unsigned *)(p.work_counter + 1);
    if (h->rows_ws.alloc((size_t)h->max_grid * 4 * p.Mpad) != hipSuccess) return fail(HMPC_EDEVICE, "cannot allocate the row workspace");
    if (getenv("HMPC_TRACE")) {
        (void)h->trace.alloc(2 * 64 * 8 + 32);
        (void)hipMemset(h->trace, 0, (2 * 64 * 8 + 32) * sizeof(double));
    }
    return HMPC_OK;
}

} // namespace

static int hmpc_certify_setup(hmpc_handle *h, int cus);

extern "C" int hmpc_create(const hmpc_problem *q, const hmpc_options *opt, hmpc_handle **out)
{
    hmpc_install_backtrace();
    g_err.clear();
    if (!q || !out) return fail(HMPC_EINVAL, "null problem or output pointer");
    HostProblem hp;
    int rc = build_host_problem(*q, opt, hp);
    if (rc) return rc;
    int dev = opt ? opt->device : -1;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return fail(HMPC_EDEVICE, "no HIP device available");
    if (hipSetDevice(dev) != hipSuccess) return fail(HMPC_EDEVICE, "hipSetDevice failed");
    std::unique_ptr<hmpc_handle> h(new hmpc_handle());
    h->device = dev;
    h->dp = hp.p;
    // launch geometry: one 64-lane workgroup per node in flight, as many per CU as LDS admits
    int cus = 0, lds_max = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    if ((rc = choose_kernels(h->dp, lds_max, h->cfg, h->jit_libs, h->jit_kernels, nullptr))) return rc;
    if ((rc = setup_device(h.get(), hp, *q, cus, lds_max))) return rc;
    if ((rc = hmpc_certify_setup(h.get(), cus))) return rc;
    *out = h.release();
    return HMPC_OK;
}

// What hmpc_create would compile for this problem -- the register kernels of its shape, or the run-time-sized kernel with
// its sizes (hmpc_jit.h) --, compiled into the cache WITHOUT a GPU: packaging, or warming the cache of a machine without a
// compiler from one that has it.  The host side of hmpc_create up to the choice of kernels; nothing is uploaded or loaded.
// paths (may be NULL): the shared objects, newline separated.
extern "C" int hmpc_jit_build_problem(const hmpc_problem *q, const hmpc_options *opt, char *paths, int32_t paths_len)
{
    g_err.clear();
    if (!q) return fail(HMPC_EINVAL, "null problem or output pointer");
    HostProblem hp;
    int rc = build_host_problem(*q, opt, hp);
    if (rc) return rc;
    hmpc_cfg cfg[3];
    std::vector<void *> libs;
    std::vector<std::string> built;
    int jit_kernels = 0;
    if ((rc = choose_kernels(hp.p, 0, cfg, libs, jit_kernels, &built))) return rc;
    if (paths && paths_len > 0) {
        std::string all;
        for (const std::string &b : built) all += b + "\n";
        snprintf(paths, (size_t)paths_len, "%s", all.c_str());
    }
    return HMPC_OK;
}

extern "C" int hmpc_destroy(hmpc_handle *h)
{
    if (!h) return HMPC_OK;
    (void)hipSetDevice(h->device);
    // (work this handle issued on a caller's stream may still be in flight -- the counts of a second opinion travel to pinned
    // memory behind an event nobody has waited for: everything on the device ends before anything is freed)
    (void)hipDeviceSynchronize();
    delete h;
    return HMPC_OK;
}

// Which kind of kernel serves this problem, per waves per node (1, 2, 4): 0 run-time-sized, 1 its streaming form,
// 2 built-in register kernel, 4 / 5 / 6 the run-time-sized kernel / its streaming form / the register kernel compiled with
// this problem's sizes at hmpc_create (3, the register kernel compiled per SHAPE of round 4, no longer exists).
extern "C" int hmpc_kernel_info(const hmpc_handle *h, int32_t *kind3)
{
    if (!h || !kind3) return fail(HMPC_EINVAL, "null argument");
    for (int c = 0; c < 3; c++) {
        const hmpc_kernel_choice &k = h->cfg[c].k;
        kind3[c] = k.kc > 0 ? (h->cfg[c].sized ? 6 : 2) : (k.big ? 1 : 0) + (h->cfg[c].sized ? 4 : 0);
    }
    return HMPC_OK;
}

// Which compiled kernels of this handle (1 / 2 / 4 waves per node) were built with the compiler's ILP schedule -- binaries listed in the
// cache's VALIDATED manifest (csrc/hmpc_jit.h) --; 0: the default schedule, or a shipped kernel.
extern "C" int hmpc_kernel_recipe(const hmpc_handle *h, int32_t *ilp3)
{
    if (!h || !ilp3) return fail(HMPC_EINVAL, "null argument");
    for (int c = 0; c < 3; c++) ilp3[c] = h->cfg[c].sized ? h->cfg[c].ilp : 0;
    return HMPC_OK;
}

// Compiled kernels of this handle: how many were dropped by the first-use check or the second opinion, in how many solve calls
// the shipped kernel was asked for a second opinion, and on how many of those batches it ended like the compiled one.
extern "C" int hmpc_jit_stats(const hmpc_handle *h, int32_t *dropped, int32_t *second_runs, int32_t *second_agreed)
{
    if (!h) return fail(HMPC_EINVAL, "null handle");
    if (dropped) *dropped = h->jit_rejected;
    if (second_runs) *second_runs = h->second_runs;
    if (second_agreed) *second_agreed = h->cfg[0].second_opinions + h->cfg[1].second_opinions + h->cfg[2].second_opinions;
    return HMPC_OK;
}

extern "C" int hmpc_record_sizes(const hmpc_handle *h, int32_t *n_primal, int32_t *n_dual)
{
    if (!h) return fail(HMPC_EINVAL, "null handle");
    if (n_primal) *n_primal = h->dp.n_primal;
    if (n_dual) *n_dual = h->dp.n_dual;
    return HMPC_OK;
}

extern "C" int hmpc_set_shift_maps(hmpc_handle *h, const hmpc_shift_maps *m)
{
    g_err.clear();
    if (!h || !m || !m->M_mu || !m->M_rho || !m->V) return fail(HMPC_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->device));
    DevProb &p = h->dp;
    // the retain rule of the shift kernel reads one binary per lane of a wavefront
    if (p.nub > 64) return fail(HMPC_EINVAL, "the node shift supports at most 64 binaries per stage");
    // a second call replaces the maps (the previous device copies are released)
    h->shift_blocks.clear();
    p.shift_Mmu = p.shift_Mrho = p.shift_V = h->shift_MT2 = nullptr;
    // M_mu also in pairs of columns: [pair][row] -> (column 2k, column 2k + 1), an odd last column paired with zeros
    const size_t ncL2 = ((size_t)p.ncL + 1) / 2;
    std::vector<double> mt(2 * ncL2 * p.nc, 0.0);
    for (int r = 0; r < p.nc; r++)
        for (int k = 0; k < p.ncL; k++) mt[((size_t)(k / 2) * p.nc + r) * 2 + (k & 1)] = m->M_mu[(size_t)r * p.ncL + k];
    auto vec = [](const double *a, size_t n) { return std::vector<double>(a, a + n); };
    Uploader up{h->shift_blocks};
    up(vec(m->M_mu, (size_t)p.nc * p.ncL), p.shift_Mmu);
    up(vec(m->M_rho, (size_t)p.nq * p.nqT), p.shift_Mrho);
    up(vec(m->V, (size_t)p.nub * p.nu), p.shift_V);
    up(mt, h->shift_MT2);
    return up.rc;
}

static int hmpc_launch_shift(hmpc_handle *h, const ShiftArgs &a, void *stream);

extern "C" int hmpc_shift_batch_device(hmpc_handle *h, int32_t B, int32_t K, const int32_t *d_owner, const double *d_x0,
                                       const double *d_u0, const double *d_e0, const int8_t *d_fix, const double *d_lb,
                                       const double *d_dual, const double *d_dual_obj, int8_t *d_fix_out, double *d_lb_out,
                                       double *d_dual_out, double *d_dual_obj_out, uint8_t *d_flags, void *stream)
{
    g_err.clear();
    if (!h) return fail(HMPC_EINVAL, "null handle");
    if (!h->dp.shift_Mmu) return fail(HMPC_EINVAL, "hmpc_set_shift_maps has not been called");
    if (B < 0 || K < 1) return fail(HMPC_EINVAL, "bad leaf or tree count");
    if (B == 0) return HMPC_OK;
    if (!d_owner || !d_x0 || !d_u0 || !d_e0 || !d_fix || !d_lb || !d_dual || !d_dual_obj || !d_fix_out || !d_lb_out ||
        !d_dual_out || !d_dual_obj_out || !d_flags)
        return fail(HMPC_EINVAL, "null argument");
    if (d_dual == d_dual_out || d_fix == d_fix_out) return fail(HMPC_EINVAL, "the shift is not in place");
    HIPCHK(hipSetDevice(h->device));
    ShiftArgs a{B, K, d_owner, d_x0, d_u0, d_e0, d_fix, d_lb, d_dual, d_dual_obj, nullptr, d_fix_out, d_lb_out, d_dual_out, d_dual_obj_out, d_flags};
    return hmpc_launch_shift(h, a, stream);
}

// (shared with the fleet driver, which passes a row indirection)
static int hmpc_launch_shift(hmpc_handle *h, const ShiftArgs &a, void *stream)
{
    const int B = a.B;
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device);
    {   // rows staged in LDS by the memory pipeline (hmpc_shift.hip, second kernel): one workgroup per CU, a row buffer per wave
        const char *rows_env = getenv("HMPC_SHIFT_ROWS");   // (read per launch: the tests run both kernels in one process)
        const bool off = rows_env && atoi(rows_env) == 0;
        static const int cap = getenv("HMPC_SHIFT_ROW_WAVES") ? atoi(getenv("HMPC_SHIFT_ROW_WAVES")) : 0;   // (diagnostic)
        const size_t fixed = hmpc_shift_row_fixed_doubles(h->dp), per = hmpc_shift_row_wave_doubles(h->dp), room = 160 * 1024 / sizeof(double);
        int waves = fixed < room ? (int)((room - fixed) / per) : 0;
        if (waves > 16) waves = 16;
        if (cap > 0 && cap < waves) waves = cap;
        const DevProb &q = h->dp;
        if (!off && h->shift_MT2 && waves >= 4 && q.n_dual >= 2 && q.nub >= 1 && q.nc >= 1 && q.ncL >= 1 && q.nq >= 1 && q.nr >= 1 && q.nx >= 1) {
            const size_t lds = (fixed + (size_t)waves * per) * sizeof(double), need_tv = (size_t)a.K * hmpc_shift_tree_doubles(q);
            HIPCHK(h->shift_tv.grow(need_tv, need_tv, (hipStream_t)stream)); // (with the number of trees: the stream's earlier launches still read the old block)
            int grid = cus > 0 ? cus : 256;
            const int need = (B + waves - 1) / waves;
            if (grid > need) grid = need;
            if (hipFuncSetAttribute((const void *)hmpc_shift_row_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) {
                hipLaunchKernelGGL(hmpc_shift_tree_kernel, dim3(a.K), dim3(64), 0, (hipStream_t)stream, h->dp, a.K, a.x0, a.u0, h->shift_tv);
                hipLaunchKernelGGL(hmpc_shift_row_kernel, dim3(grid), dim3(64 * waves), lds, (hipStream_t)stream, h->dp, a, (const double *)h->shift_tv, (const double2 *)h->shift_MT2);
                HIPCHK(hipGetLastError());
                return HMPC_OK;
            }
            (void)hipGetLastError();
        }
    }
    // persistent workgroups: enough to fill the device, each wave walks leaves with stride grid * SHIFT_WAVES
    const bool staged = hmpc_shift_lds_doubles(h->dp, true) * sizeof(double) <= 64 * 1024;
    const size_t lds = hmpc_shift_lds_doubles(h->dp, staged) * sizeof(double);
    int per_cu = (int)((160 * 1024) / (lds > 0 ? lds : 1));
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) return fail(HMPC_ETOOBIG, "the shift's last-stage vectors exceed one CU's LDS");
    int grid = (cus > 0 ? cus : 256) * per_cu;
    const int need = (B + SHIFT_WAVES - 1) / SHIFT_WAVES;
    if (grid > need) grid = need;
    if (staged) {
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void *)hmpc_shift_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(hmpc_shift_kernel<true>, dim3(grid), dim3(64 * SHIFT_WAVES), lds, (hipStream_t)stream, h->dp, a);
    } else {
        hipLaunchKernelGGL(hmpc_shift_kernel<false>, dim3(grid), dim3(64 * SHIFT_WAVES), lds, (hipStream_t)stream, h->dp, a);
    }
    HIPCHK(hipGetLastError());
    return HMPC_OK;
}

extern "C" int hmpc_shift_batch(hmpc_handle *h, int32_t B, int32_t K, const int32_t *owner, const double *x0, const double *u0,
                                const double *e0, const int8_t *fix, const double *lb, const double *dual, const double *dual_obj,
                                int8_t *fix_out, double *lb_out, double *dual_out, double *dual_obj_out, uint8_t *flags)
{
    g_err.clear();
    if (!h) return fail(HMPC_EINVAL, "null handle");
    if (B < 0 || K < 1) return fail(HMPC_EINVAL, "bad leaf or tree count");
    if (B == 0) return HMPC_OK;
    if (!owner || !x0 || !u0 || !e0 || !fix || !lb || !dual || !dual_obj || !fix_out || !lb_out || !dual_out || !dual_obj_out || !flags)
        return fail(HMPC_EINVAL, "null argument");
    HIPCHK(hipSetDevice(h->device));
    const DevProb &p = h->dp;
    const size_t nf = (size_t)B * p.T * p.nub, nd = (size_t)B * p.n_dual * sizeof(double), nb = (size_t)B * sizeof(double);
    // one staging block: inputs then outputs
    struct Part { size_t bytes; const void *src; void *dst; size_t off; };
    Part parts[] = {{(size_t)B * 4, owner, nullptr, 0}, {(size_t)K * p.nx * 8, x0, nullptr, 0}, {(size_t)K * p.nu * 8, u0, nullptr, 0},
                    {(size_t)K * p.nx * 8, e0, nullptr, 0}, {nf, fix, nullptr, 0}, {nb, lb, nullptr, 0}, {nd, dual, nullptr, 0},
                    {nb, dual_obj, nullptr, 0}, {nf, nullptr, fix_out, 0}, {nb, nullptr, lb_out, 0}, {nd, nullptr, dual_out, 0},
                    {nb, nullptr, dual_obj_out, 0}, {(size_t)B, nullptr, flags, 0}};
    size_t total = 0;
    for (Part &q : parts) { q.off = total; total += (q.bytes + 255) / 256 * 256; }
    HIPCHK(h->d_shift.grow(total, total, nullptr));
    char *base = (char *)h->d_shift;
    for (const Part &q : parts)
        if (q.src) HIPCHK(hipMemcpyAsync(base + q.off, q.src, q.bytes, hipMemcpyHostToDevice, 0));
    const int rc = hmpc_shift_batch_device(h, B, K, (const int32_t *)(base + parts[0].off), (const double *)(base + parts[1].off),
                                           (const double *)(base + parts[2].off), (const double *)(base + parts[3].off),
                                           (const int8_t *)(base + parts[4].off), (const double *)(base + parts[5].off),
                                           (const double *)(base + parts[6].off), (const double *)(base + parts[7].off),
                                           (int8_t *)(base + parts[8].off), (double *)(base + parts[9].off),
                                           (double *)(base + parts[10].off), (double *)(base + parts[11].off),
                                           (uint8_t *)(base + parts[12].off), nullptr);
    if (rc != HMPC_OK) return rc;
    for (const Part &q : parts)
        if (q.dst) HIPCHK(hipMemcpyAsync(q.dst, base + q.off, q.bytes, hipMemcpyDeviceToHost, 0));
    HIPCHK(hipStreamSynchronize(0));
    return HMPC_OK;
}

extern "C" int hmpc_launch_info(const hmpc_handle *h, int32_t *grid, int32_t *lds_bytes)
{
    if (!h) return fail(HMPC_EINVAL, "null handle");
    if (grid) *grid = h->last_grid;
    if (lds_bytes) *lds_bytes = (int32_t)h->lds;
    return HMPC_OK;
}

// FIRST-USE CHECK of a kernel compiled at hmpc_create (hmpc_cfg::ref).  The run-time compiler produces code nobody has run
// before for a problem nobody has seen -- and this kernel lives at the edge of the register file (round 5 traced the wrong
// binaries of round 4 to the compiler's stack-slot colouring of spilled scalars: DESIGN.md 4.8).  So the first launch through a
// configuration solves HMPC_CHECK_NODES nodes -- spread over ITS batch, plus the root relaxation and the deepest node of the
// batch's first initial state (hmpc_check_set_kernel) -- with the compiled kernel and with the shipped kernel of the same wave
// count, and compares statuses and objectives (1e-6 relative: the two are the same algorithm).  Agreement: the compiled
// kernel serves from then on.  Disagreement: it is dropped for this handle, loudly.  One stream synchronisation, once per
// configuration (hmpc_validate_kernels runs it ahead of time: a caller that captures its stream, or must not block in a solve call).
static int hmpc_check_compiled(hmpc_handle *h, hmpc_cfg &cf, const double *d_x0, int x0_stride, const int8_t *d_fix, int B, hipStream_t stream)
{
    cf.checked = 1;
    if (!cf.ref.fn || !h->chk || h->trace) return HMPC_OK;
    if (getenv("HMPC_JIT_SELFCHECK_SKIP_FIRST")) return HMPC_OK; // (test hook: leaves a wrong kernel to the second opinion of hmpc_solve_batch_device)
    constexpr int N = HMPC_CHECK_NODES;
    const DevProb &p = h->dp;
    const int nfix = p.T * p.nub;
    const CheckLayout L = check_layout(p);
    char *d = h->chk;
    double *obj = (double *)(d + L.obj), *dobj = (double *)(d + L.dobj);
    int32_t *st = (int32_t *)(d + L.status), *it = (int32_t *)(d + L.iters), *idx = (int32_t *)(d + L.idx);
    double *prim = (double *)(d + L.primal), *dual = (double *)(d + L.dual), *x0c = (double *)(d + L.x0);
    int8_t *fixc = (int8_t *)(d + L.fix);
    hipLaunchKernelGGL(hmpc_check_set_kernel, dim3(N), dim3(256), 0, stream, d_x0, x0_stride, d_fix, B, nfix, p.nx, N, x0c, fixc);
    HIPCHK(hipGetLastError());
    const DevWarm w{nullptr, nullptr, nullptr, nullptr, 0};
    // runs 0 / 1: the shipped and the compiled kernel, cold (the compiled one keeps its records for run 2)
    for (int which = 0; which < 2; which++) {
        const hmpc_kernel_choice &k = which ? cf.k : cf.ref;
        const size_t lds = which ? cf.lds : cf.ref_lds;
        const int grid = N < (which ? cf.max_grid : cf.ref_grid) ? N : (which ? cf.max_grid : cf.ref_grid);
        const DevOut o{obj + which * N, dobj + which * N, st + which * N, it + which * N, which ? prim : nullptr, which ? dual : nullptr};
        HIPCHK(hipMemsetAsync(h->dp.work_counter, 0, sizeof(int), stream));
        hipLaunchKernelGGL(k.fn, dim3(grid), dim3(64 * k.waves), lds, stream, h->dp, x0c, p.nx, fixc, N, o, h->rows_ws, (double *)nullptr,
                           (const int32_t *)nullptr, w);
        HIPCHK(hipGetLastError());
    }
    if (!h->h_chk) return HMPC_OK;
    char *hm = h->h_chk;   // (pinned, see setup_device)
    double *hobj = (double *)(hm + L.obj), *hdob = (double *)(hm + L.dobj);
    int32_t *hst = (int32_t *)(hm + L.status), *hidx = (int32_t *)(hm + L.idx);
    HIPCHK(hipMemcpyAsync(hobj, obj, 2 * N * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(hdob, dobj, 2 * N * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(hst, st, 2 * N * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    bool same = true;
    for (int b = 0; b < N; b++) {
        const int sa = hst[b], sb = hst[N + b];
        // (a node the SHIPPED kernel leaves undecided decides nothing about the compiled one)
        same = same && (sa == sb || sa >= HMPC_MAXITER);
        if (sa == HMPC_OPTIMAL && sb == HMPC_OPTIMAL) {
            const double a = hobj[b], c = hobj[N + b];
            same = same && std::fabs(a - c) <= 1e-6 * (1.0 + std::fabs(a));
        }
        // (an infeasible node's ray is normalised to a unit largest entry: its dual objective is a scalar of the WHOLE ray -- the
        // one wrong binary round 5 met that was not loud had right statuses and rays scaled by 1e-43, dual objectives off by 1e-2)
        if (sa == HMPC_INFEASIBLE && sb == HMPC_INFEASIBLE) {
            const double a = hdob[b], c = hdob[N + b];
            same = same && (std::fabs(a - c) <= 1e-4 * std::fabs(a) + 1e-9) && c == c;
        }
    }
    // run 2: the HAND-DOWN instantiation of the compiled kernel (its own binary), every optimal node handed its own record:
    // same statuses, same objectives, and a polished node's active set verifies without an interior-point iteration
    if (same && cf.k.fn_warm) {
        for (int b = 0; b < N; b++) hidx[b] = hst[N + b] == HMPC_OPTIMAL ? b : -1;
        HIPCHK(hipMemcpyAsync(idx, hidx, N * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        const DevWarm ww{prim, dual, idx, nullptr, 0};
        const DevOut o{obj + 2 * N, dobj + 2 * N, st + 2 * N, it + 2 * N, nullptr, nullptr};
        HIPCHK(hipMemsetAsync(h->dp.work_counter, 0, sizeof(int), stream));
        hipLaunchKernelGGL(cf.k.fn_warm, dim3(N < cf.max_grid ? N : cf.max_grid), dim3(64 * cf.k.waves), cf.lds, stream, h->dp, x0c, p.nx, fixc, N, o, h->rows_ws,
                           (double *)nullptr, (const int32_t *)nullptr, ww);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hobj + 2 * N, obj + 2 * N, N * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(hst + 2 * N, st + 2 * N, N * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        for (int b = 0; b < N; b++) {
            same = same && (hst[2 * N + b] == hst[N + b] || hst[N + b] >= HMPC_MAXITER);
            if (hst[N + b] == HMPC_OPTIMAL && hst[2 * N + b] == HMPC_OPTIMAL)
                same = same && std::fabs(hobj[2 * N + b] - hobj[N + b]) <= 1e-6 * (1.0 + std::fabs(hobj[N + b]));
        }
    }
    if (getenv("HMPC_JIT_SELFCHECK_FAIL")) same = false; // (test hook: the path a disagreement takes)
    if (!same) {
        fprintf(stderr, "hmpc: the kernel compiled for this problem (%d waves per node) disagrees with the shipped kernel on the %d nodes of its first-use check: "
                        "dropped, the shipped kernel serves this handle (please report; HMPC_JIT_SIZED=0 / HMPC_JIT=0 avoid the compilation)\n", cf.k.waves, N);
        cf.k = cf.ref;
        cf.lds = cf.ref_lds;
        cf.max_grid = cf.ref_grid;
        cf.sized = 0;
        cf.ilp = 0;
        cf.checked = -1;
        h->jit_rejected++;
    }
    return HMPC_OK;
}

// The counts of the last second opinion, if they have arrived (never blocks unless `wait`): a compiled kernel that left nodes
// undecided of which the shipped kernel decides some is dropped for the handle; three batches on which both end the same way
// and the compiled kernel is trusted with its hard nodes (no further second launches for that configuration).
static void hmpc_second_opinion_review_impl(hmpc_handle *h, bool wait)
{
    if (h->hard_cfg < 0 || !h->hard_done) return;
    if (wait) { if (hipEventSynchronize(h->hard_done) != hipSuccess) return; }
    else if (hipEventQuery(h->hard_done) != hipSuccess) { (void)hipGetLastError(); return; }
    hmpc_cfg &cc = h->cfg[h->hard_cfg];
    h->hard_cfg = -1;
    const int after = h->h_hard[0], first = h->h_hard[1];
    if (first <= 0 || !cc.ref.fn || cc.k.fn == cc.ref.fn) return;
    if (after < first) {
        fprintf(stderr, "hmpc: the kernel compiled for this problem (%d waves per node) left %d nodes of a batch undecided of which the shipped kernel decides %d: "
                        "dropped, the shipped kernel serves this handle (please report; HMPC_JIT_SIZED=0 / HMPC_JIT=0 avoid the compilation)\n",
                cc.k.waves, first, first - after);
        cc.k = cc.ref;
        cc.lds = cc.ref_lds;
        cc.max_grid = cc.ref_grid;
        cc.sized = 0;
        cc.ilp = 0;
        cc.checked = -1;
        h->jit_rejected++;
    } else {
        cc.second_opinions++;
    }
}

extern "C" int hmpc_second_opinion_review(hmpc_handle *h)
{
    if (!h) return fail(HMPC_EINVAL, "null handle");
    hmpc_second_opinion_review_impl(h, true);
    return HMPC_OK;
}

// Runs the first-use checks of all three configurations now (one synchronisation each) instead of inside the first solve call
// through each: for callers that capture their stream in a graph or must not block there.  x0 / fix: any batch of the problem.
extern "C" int hmpc_validate_kernels(hmpc_handle *h, const double *d_x0, int32_t x0_stride, const int8_t *d_fix, int32_t B, void *stream)
{
    g_err.clear();
    if (!h || !d_x0 || !d_fix || B < 1) return fail(HMPC_EINVAL, "null argument or empty batch");
    HIPCHK(hipSetDevice(h->device));
    for (int c = 0; c < 3; c++)
        if (!h->cfg[c].checked) {
            const int rc = hmpc_check_compiled(h, h->cfg[c], d_x0, x0_stride, d_fix, B, (hipStream_t)stream);
            if (rc != HMPC_OK) return rc;
        }
    return HMPC_OK;
}

extern "C" int hmpc_solve_batch_device(hmpc_handle *h, const double *d_x0, int32_t x0_stride, const int8_t *d_fix,
                                       int32_t B, const hmpc_warm *d_warm, const hmpc_result *d_out, void *stream)
{
    g_err.clear();
    if (!h || !d_x0 || !d_fix || !d_out) return fail(HMPC_EINVAL, "null argument");
    if (B < 0 || (x0_stride != 0 && x0_stride < h->dp.nx)) return fail(HMPC_EINVAL, "bad batch size or x0 stride");
    if (B == 0) return HMPC_OK;
    HIPCHK(hipSetDevice(h->device));
    hmpc_second_opinion_review_impl(h, false);
    DevOut o{d_out->obj, d_out->dual_obj, d_out->status, d_out->iters, d_out->primal, d_out->dual};
    DevWarm w{nullptr, nullptr, nullptr, nullptr, 0};
    if (d_warm && d_warm->index) {
        if (!d_warm->primal || !d_warm->dual) return fail(HMPC_EINVAL, "hmpc_warm: index without record rows");
        w = DevWarm{d_warm->primal, d_warm->dual, d_warm->index, nullptr, 0};
    }
    int nw = hmpc_waves_for(B, h->cfg[0].max_grid);
    // the streaming form holds one node per CU whatever the number of waves: always spread it over all four SIMDs
    if (h->cfg[2].k.big && !getenv("HMPC_WAVES")) nw = 4;
    hmpc_cfg &cfm = h->cfg[nw == 1 ? 0 : nw == 2 ? 1 : 2];
    h->last_cfg = nw == 1 ? 0 : nw == 2 ? 1 : 2;
    if (!cfm.checked) {
        const int rc = hmpc_check_compiled(h, cfm, d_x0, x0_stride, d_fix, B, (hipStream_t)stream);
        if (rc != HMPC_OK) return rc;
    }
    const hmpc_cfg &cf = cfm;
    const hmpc_kernel_choice &k = cf.k;
    const int grid = B < cf.max_grid ? B : cf.max_grid;
    h->last_grid = grid;
    h->lds = cf.lds;
    // (every launch: also a launch with B <= grid reads the counter once per workgroup, and what it reads must be >= 0)
    HIPCHK(hipMemsetAsync(h->dp.work_counter, 0, sizeof(int), (hipStream_t)stream));
    // more nodes than resident workgroups: hand them out shallow first (hmpc_order_kernel)
    int32_t *order = nullptr;
    if (B > grid + grid / 8 && !getenv("HMPC_NO_ORDER")) {
        HIPCHK(h->order.grow(B, B + B / 2, (hipStream_t)stream));
        order = h->order;
        hipLaunchKernelGGL(hmpc_order_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, d_fix, B, h->dp.T * h->dp.nub, order, w,
                           (h->dp.T + 1) * h->dp.nx + (h->dp.T - 1) * h->dp.nc + h->dp.nc, h->dp.nT, h->dp.n_dual);
    }
    // TWO-LAUNCH FORM of the lazy terminal set (DevWarm; round 4; OPT-IN: HMPC_SPLIT=1): a large cold batch of a register
    // kernel with one wave per node.  A node that needs the terminal-set rows takes 24+ iterations where the others take
    // 7 - 12, and at one wave per node it is the tail of the launch wherever it starts (6 % of the nodes of real closed-loop
    // trees: 12.4 ms per 4096 nodes against 9.0 without them).  The first launch leaves those nodes to a second one: four
    // waves per node, each from its own first record -- the active set of the masked solve plus the terminal rows it
    // violates: 232 of 238 such nodes verify that way in a few rounds (11.5 instead of 13.6 iterations per optimal node).
    // Same statuses, same vertices (1e-9).  MEASURED SLOWER, which is why it is not the default: 13.05 ms against 12.44 --
    // the six nodes whose own set does not verify (infeasible with the terminal set: they owe a certificate) run a full
    // second solve, 24 iterations = 3 ms even at four waves, ALONE on the device: the tail has moved into a launch of its
    // own.  What would pay is knowing those nodes before their first solve (profiles/r04_split.txt).
    const hmpc_cfg &c4 = h->cfg[2];
    const bool split = !w.index && nw == 1 && k.kc > 0 && c4.k.kc > 0 && h->dp.nT > 0 && h->dp.lazy && h->dp.polish && o.primal && o.dual && o.iters &&
                       o.status && getenv("HMPC_SPLIT") && !h->trace;
    if (split) {
        HIPCHK(h->pend.grow(B + 1, B + B / 2 + 1, (hipStream_t)stream));
        HIPCHK(hipMemsetAsync(h->pend, 0, sizeof(int32_t), (hipStream_t)stream));
        w.pend = h->pend;
    }
    hipLaunchKernelGGL(w.index ? k.fn_warm : k.fn, dim3(grid), dim3(64 * k.waves), cf.lds, (hipStream_t)stream, h->dp, d_x0, x0_stride,
                       d_fix, B, o, h->rows_ws, h->trace, (const int32_t *)order, w);
    HIPCHK(hipGetLastError());
    if (split) {
        // (how many nodes wait is known on the device only: enough workgroups for all of them, those without a node leave at once)
        const int grid2 = B < c4.max_grid ? B : c4.max_grid;
        HIPCHK(hipMemsetAsync(h->dp.work_counter, 0, sizeof(int), (hipStream_t)stream));
        DevWarm w2{o.primal, o.dual, nullptr, h->pend, 1};
        hipLaunchKernelGGL(c4.k.fn_warm, dim3(grid2), dim3(64 * c4.k.waves), c4.lds, (hipStream_t)stream, h->dp, d_x0, x0_stride, d_fix, B, o, h->rows_ws,
                           h->trace, (const int32_t *)nullptr, w2);
        HIPCHK(hipGetLastError());
    }
    // SECOND OPINION on a kernel compiled at hmpc_create (binaries of this kernel have come out wrong from the
    // compiler, always loudly -- nodes ending NUMERICAL -- and the reference never hands back an undecided node,
    // bounded_qp.py:216-228): the nodes such a kernel leaves MAXITER / NUMERICAL are listed on the device (hmpc_hard_kernel)
    // and solved again, in the same stream, by the SHIPPED kernel of the wave count (its hand-down instantiation in list mode,
    // DevWarm::second == 2; a node is handed what the first launch handed it); its records replace theirs.  Nothing is
    // synchronised: with no such node -- every call so far of every default kernel -- the two launches end at once (~10 us).
    // The counts travel to the host behind an event and are looked at by the next call (hmpc_second_opinion_review_impl).
    // Every entry that solves goes through here: hmpc_solve_batch, hmpc_fleet_solve, callers with device pointers.
    if (cfm.ref.fn && k.fn != cfm.ref.fn && cfm.ref.fn_warm && o.status && !h->trace && !split && cfm.second_opinions < 3 && h->hard_done) {
        HIPCHK(h->hard.grow(B + 4, B + B / 2 + 4, (hipStream_t)stream));
        HIPCHK(hipMemsetAsync(h->hard, 0, 3 * sizeof(int32_t), (hipStream_t)stream));
        hipLaunchKernelGGL(hmpc_hard_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const int32_t *)o.status, B, h->hard + 2);
        HIPCHK(hipGetLastError());
        DevProb p2 = h->dp;
        p2.work_counter = h->hard + 1;
        const int g2 = B < 64 ? B : 64; // (hard nodes are few; more of them than workgroups are handed out through the counter)
        const DevWarm w3{w.primal, w.dual, w.index, h->hard + 2, 2};
        hipLaunchKernelGGL(cfm.ref.fn_warm, dim3(g2 < cfm.ref_grid ? g2 : cfm.ref_grid), dim3(64 * cfm.ref.waves), cfm.ref_lds, (hipStream_t)stream, p2, d_x0, x0_stride,
                           d_fix, B, o, h->rows_ws, (double *)nullptr, (const int32_t *)nullptr, w3);
        HIPCHK(hipGetLastError());
        h->second_runs++;
        if (h->hard_cfg < 0) { // (the counts of an earlier call still in flight: this call's are not looked at)
            HIPCHK(hipMemcpyAsync(h->h_hard, h->hard, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
            HIPCHK(hipMemcpyAsync(h->h_hard + 1, h->hard + 2, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
            HIPCHK(hipEventRecord(h->hard_done, (hipStream_t)stream));
            h->hard_cfg = h->last_cfg;
        }
    }
    return HMPC_OK;
}

// Staging of the host-pointer entry point: ONE device block and ONE pinned host block, inputs first, then the outputs in
// the order obj | dual_obj | status | iters | primal | dual -- one copy up, one copy down per call (round 1: two pageable
// copies up, six down, each its own synchronisation: ~100 us of a 1.4 ms branch-and-bound round).
struct StageLayout {
    size_t x0, fix, widx, wprim, wdual, obj, dobj, status, iters, primal, dual, in_bytes, total;
};
// nw: parent records handed down with the batch (gathered: one row per node that has one)
static StageLayout stage_layout(const DevProb &p, size_t B, size_t nw = 0)
{
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    StageLayout L;
    L.x0 = 0;
    L.fix = up(B * p.nx * sizeof(double));
    L.widx = L.fix + up(B * (size_t)p.T * p.nub + 1);
    L.wprim = L.widx + (nw ? up(B * sizeof(int32_t)) : 0);
    L.wdual = L.wprim + up(nw * (size_t)p.n_primal * sizeof(double));
    L.in_bytes = L.wdual + up(nw * (size_t)p.n_dual * sizeof(double));
    L.obj = L.in_bytes;
    L.dobj = L.obj + up(B * sizeof(double));
    L.status = L.dobj + up(B * sizeof(double));
    L.iters = L.status + up(B * sizeof(int32_t));
    L.primal = L.iters + up(B * sizeof(int32_t));
    L.dual = L.primal + up(B * (size_t)p.n_primal * sizeof(double));
    L.total = L.dual + up(B * (size_t)p.n_dual * sizeof(double));
    return L;
}

// Room in both staging blocks for a batch of B nodes, nw of them with a parent record; a block that is short is replaced by one
// for 64 nodes, or B + B / 4 from 64 on (each with room for a record if any of this batch has one)
static int ensure_staging(hmpc_handle *h, size_t B, size_t nw)
{
    const size_t cap = B < 64 ? 64 : B + B / 4;
    const size_t want = stage_layout(h->dp, B, nw).total, room = stage_layout(h->dp, cap, nw ? cap : 0).total;
    HIPCHK(h->d_stage.grow(want, room, nullptr));
    HIPCHK(h->h_stage.grow(want, room, nullptr));
    return HMPC_OK;
}

extern "C" int hmpc_solve_batch(hmpc_handle *h, const double *x0, int32_t x0_stride, const int8_t *fix, int32_t B,
                                const hmpc_warm *warm, const hmpc_result *out)
{
    g_err.clear();
    if (!h || !x0 || !fix || !out) return fail(HMPC_EINVAL, "null argument");
    if (B < 0 || (x0_stride != 0 && x0_stride < h->dp.nx)) return fail(HMPC_EINVAL, "bad batch size or x0 stride");
    if (B == 0) return HMPC_OK;
    HIPCHK(hipSetDevice(h->device));
    const DevProb &p = h->dp;
    // parent records handed down: gathered, one row per node that has one (the index is rewritten to the gathered rows)
    size_t nwarm = 0;
    if (warm && warm->index) {
        if (!warm->primal || !warm->dual) return fail(HMPC_EINVAL, "hmpc_warm: index without record rows");
        for (int b = 0; b < B; b++) {
            if (warm->index[b] >= warm->rows) return fail(HMPC_EINVAL, "hmpc_warm: index beyond the rows handed in");
            nwarm += warm->index[b] >= 0;
        }
    }
    int rc = ensure_staging(h, (size_t)B, nwarm);
    if (rc) return rc;
    // offsets of THIS batch (they always fit the capacity the blocks were allocated for): with the capacity's offsets
    // a small branch-and-bound round after one large call dragged the whole capacity-sized primal region along
    const StageLayout L = stage_layout(p, (size_t)B, nwarm);
    char *hs = h->h_stage, *ds = h->d_stage;
    const size_t nfix = (size_t)p.T * p.nub;
    if (x0_stride == 0) std::memcpy(hs + L.x0, x0, p.nx * sizeof(double));
    else
        for (int b = 0; b < B; b++) std::memcpy(hs + L.x0 + (size_t)b * p.nx * sizeof(double), x0 + (size_t)b * x0_stride, p.nx * sizeof(double));
    std::memcpy(hs + L.fix, fix, (size_t)B * nfix);
    hmpc_warm dw{nullptr, nullptr, nullptr, 0};
    if (nwarm) {
        int32_t *idx = (int32_t *)(hs + L.widx);
        size_t q = 0;
        for (int b = 0; b < B; b++) {
            const int32_t r = warm->index[b];
            idx[b] = r >= 0 ? (int32_t)q : -1;
            if (r < 0) continue;
            std::memcpy(hs + L.wprim + q * p.n_primal * sizeof(double), warm->primal + (size_t)r * p.n_primal, p.n_primal * sizeof(double));
            std::memcpy(hs + L.wdual + q * p.n_dual * sizeof(double), warm->dual + (size_t)r * p.n_dual, p.n_dual * sizeof(double));
            q++;
        }
        dw = hmpc_warm{(const double *)(ds + L.wprim), (const double *)(ds + L.wdual), (const int32_t *)(ds + L.widx), (int32_t)nwarm};
    }
    HIPCHK(hipMemcpyAsync(ds, hs, L.in_bytes, hipMemcpyHostToDevice, nullptr));
    hmpc_result d{(double *)(ds + L.obj), (double *)(ds + L.dobj), (int32_t *)(ds + L.status), (int32_t *)(ds + L.iters),
                  out->primal ? (double *)(ds + L.primal) : nullptr, out->dual ? (double *)(ds + L.dual) : nullptr};
    rc = hmpc_solve_batch_device(h, (const double *)(ds + L.x0), x0_stride == 0 ? 0 : p.nx, (const int8_t *)(ds + L.fix), B,
                                 nwarm ? &dw : nullptr, &d, nullptr);
    if (rc) return rc;
    // small outputs in one copy through the pinned block; large primal / dual blocks straight into the caller's arrays
    // (a pageable copy is pipelined by the runtime, a detour through the staging block would not be)
    const size_t pbytes = (size_t)B * p.n_primal * sizeof(double), dbytes = (size_t)B * p.n_dual * sizeof(double);
    const bool big = pbytes + dbytes > (size_t)4 << 20;
    const size_t small_end = big ? L.primal : (out->dual ? L.dual + dbytes : out->primal ? L.primal + pbytes : L.primal);
    HIPCHK(hipMemcpyAsync(hs + L.obj, ds + L.obj, small_end - L.obj, hipMemcpyDeviceToHost, nullptr));
    if (big) {
        if (out->primal) HIPCHK(hipMemcpyAsync(out->primal, ds + L.primal, pbytes, hipMemcpyDeviceToHost, nullptr));
        if (out->dual) HIPCHK(hipMemcpyAsync(out->dual, ds + L.dual, dbytes, hipMemcpyDeviceToHost, nullptr));
    }
    HIPCHK(hipStreamSynchronize(nullptr));
#ifdef HMPC_CHECK
    {
        unsigned flag = 0;
        HIPCHK(hipMemcpy(&flag, h->dp.check_flag, sizeof flag, hipMemcpyDeviceToHost));
        if (flag) {
            char msg[128];
            snprintf(msg, sizeof msg, "HMPC_CHECK: in-kernel checks failed, flag bits 0x%x", flag);
            (void)hipMemset(h->dp.check_flag, 0, sizeof flag);
            return fail(HMPC_EDEVICE, msg);
        }
    }
#endif
    hmpc_second_opinion_review_impl(h, false); // (the stream is idle: the counts of this call's second opinion have arrived)
    if (out->obj) std::memcpy(out->obj, hs + L.obj, (size_t)B * sizeof(double));
    if (out->dual_obj) std::memcpy(out->dual_obj, hs + L.dobj, (size_t)B * sizeof(double));
    if (out->status) std::memcpy(out->status, hs + L.status, (size_t)B * sizeof(int32_t));
    if (out->iters) std::memcpy(out->iters, hs + L.iters, (size_t)B * sizeof(int32_t));
    if (!big) {
        if (out->primal) std::memcpy(out->primal, hs + L.primal, pbytes);
        if (out->dual) std::memcpy(out->dual, hs + L.dual, dbytes);
    }
    if (h->trace) {
        std::vector<double> tr(2 * 64 * 8 + 32);
        (void)hipMemcpy(tr.data(), h->trace, tr.size() * sizeof(double), hipMemcpyDeviceToHost);
        for (int ph = 0; ph < 2; ph++)
            for (int it = 0; it < 64; it++) {
                const double *t = &tr[(ph * 64 + it) * 8];
                if (t[0] == 0.0) break;
                fprintf(stderr, "hip ph %d it %3d tau %.3e kap %.3e mu %.3e rp %.3e rd %.3e gap %.3e eta %.3e cert %.3e\n", ph, it,
                        t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
            }
        const char *names[8] = {"residuals", "rows->D/e", "factor", "kkt_solve", "rhs aff/corr", "refine residual", "combine/step/update", "loop top"};
        for (int ph = 0; ph < 2; ph++) {
            double tot = 0;
            for (int k = 0; k < 8; k++) tot += tr[2 * 64 * 8 + ph * 8 + k];
            if (tot > 0)
                for (int k = 0; k < 8; k++)
                    fprintf(stderr, "hip stamps ph %d %-22s %12.0f cycles %5.1f%%\n", ph, names[k], tr[2 * 64 * 8 + ph * 8 + k], 100 * tr[2 * 64 * 8 + ph * 8 + k] / tot);
        }
        // (the generic kernel's solve stamps its phases as: 6 g = C'e, 7 both sweeps, 8 lam, 9 dz, 10 nu of the fixed binaries)
        const char *fn[16] = {"F gram+PA", "F assemble col", "F prescribe", "F eliminate", "F writeback+sync", "F count", "S g=C'e", "S backward", "S Minv*mu", "S forward", "S lam,dz,dnuf",
                              "W prepass", "W first chunk", "W wave 0 recursion", "W chunk barrier", "S count"};
        for (int k = 0; k < 16; k++)
            if (tr[2 * 64 * 8 + 16 + k] > 0) fprintf(stderr, "hip fine   %-22s %12.0f cycles\n", fn[k], tr[2 * 64 * 8 + 16 + k]);
        (void)hipMemset(h->trace, 0, tr.size() * sizeof(double));
    }
    return HMPC_OK;
}

// ---- Certificates of a batch of records (include/hmpc.h; kernel: hmpc_certify.hip, arithmetic: hmpc_certify.h) ----------------
static int certify_arguments(const void *x0, int32_t x0_stride, int32_t B, const hmpc_result *r, const double *residuals)
{
    if (!x0 || !r || !residuals || !r->obj || !r->dual_obj || !r->status || !r->iters || !r->primal || !r->dual)
        return fail(HMPC_EINVAL, "null argument (all six members of the records are required)");
    if (x0_stride < 0) return fail(HMPC_EINVAL, "bad x0 stride");
    return HMPC_OK;
}

// The form of the kernel for this problem, chosen ONCE at hmpc_create (the launch itself then queries nothing and sets nothing):
// 2 = rows in LDS where at least four waves' rows fit beside the matrices (one workgroup per CU), 1 = rows in place, matrices in
// LDS up to 64 KB, 0 = everything in place.  A form whose LDS this device does not grant gives way to the next one HERE, and
// form 0 needs no grant: a launch never changes form.  The limit on dynamic LDS belongs to the kernel FUNCTION, which every
// handle of the process shares, so it is set to the most any handle can ask for (form 2: all 160 KB of a CU, form 1: 64 KB of
// matrices) and never to this handle's own need: a later hmpc_create of a smaller problem leaves an earlier handle's launch its
// grant.  HMPC_CERTIFY_STAGE = 0 / 1 is a TEST switch, read at hmpc_create only: it caps the form, so that the suite runs all
// three on problems that would take one.
static int hmpc_certify_setup(hmpc_handle *h, int cus)
{
    const CertProb &c = h->cert;
    const char *env = getenv("HMPC_CERTIFY_STAGE");
    const int cap = env ? atoi(env) : 2;
    const size_t room = 160 * 1024, mats_most = 64 * 1024, mats = cert_matrix_doubles(c) * sizeof(double), per = hmpc_certify_row_doubles(c) * sizeof(double);
    h->cert_cus = cus > 0 ? cus : 256;
    h->cert_form = 0; h->cert_waves = CERT_WAVES; h->cert_lds = 0; h->cert_per_cu = 4;
    if (cap < 1 || mats > mats_most) return HMPC_OK;
    int waves = cap >= 2 ? (int)((room - mats) / per) : 0;
    if (waves > CERT_MAX_WAVES) waves = CERT_MAX_WAVES;
    if (waves >= 4) {
        const size_t lds = mats + (size_t)waves * per;
        if (hipFuncSetAttribute((const void *)hmpc_certify_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)room) == hipSuccess) {
            h->cert_form = 2; h->cert_waves = waves; h->cert_lds = lds; h->cert_per_cu = 1;
            return HMPC_OK;
        }
        (void)hipGetLastError();
    }
    if (hipFuncSetAttribute((const void *)hmpc_certify_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mats_most) == hipSuccess) {
        int per_cu = (int)(room / (mats ? mats : 1));
        h->cert_form = 1; h->cert_lds = mats; h->cert_per_cu = per_cu > 4 ? 4 : per_cu;
        return HMPC_OK;
    }
    (void)hipGetLastError();
    return HMPC_OK;
}

static int hmpc_launch_certify(hmpc_handle *h, const CertArgs &a, void *stream)
{
    const CertProb &c = h->cert;
    const hipStream_t st = (hipStream_t)stream;
    const int waves = h->cert_waves, need = (a.B + waves - 1) / waves, most = h->cert_cus * h->cert_per_cu;
    const dim3 grid(need < most ? need : most), block(64 * waves);
    if (h->cert_form == 2) hipLaunchKernelGGL((hmpc_certify_kernel<true, true>), grid, block, h->cert_lds, st, c, a);
    else if (h->cert_form == 1) hipLaunchKernelGGL((hmpc_certify_kernel<true, false>), grid, block, h->cert_lds, st, c, a);
    else hipLaunchKernelGGL((hmpc_certify_kernel<false, false>), grid, block, 0, st, c, a);
    HIPCHK(hipGetLastError());
    return HMPC_OK;
}

extern "C" int hmpc_certify_batch_device(hmpc_handle *h, const double *d_x0, int32_t x0_stride, const int8_t *d_fix, int32_t B,
                                         const hmpc_result *d_records, const hmpc_cert_tol *tol, double *d_residuals,
                                         int32_t *d_verdict, void *stream)
{
    g_err.clear();
    if (B < 0) return fail(HMPC_EINVAL, "bad batch size");
    if (h && B == 0) return HMPC_OK; // (an empty batch has no arrays to speak of: a view of an empty array may be null)
    int rc = certify_arguments(d_x0, x0_stride, B, d_records, d_residuals);
    if (rc) return rc;
    if (!h) return fail(HMPC_EINVAL, "null handle");
    if (!d_fix && h->cert.nub > 0) return fail(HMPC_EINVAL, "null argument");
    if (x0_stride != 0 && x0_stride < h->cert.nx) return fail(HMPC_EINVAL, "bad x0 stride");
    HIPCHK(hipSetDevice(h->device));
    const CertArgs a{B, x0_stride, d_x0, d_fix, d_records->obj, d_records->dual_obj, d_records->status, d_records->iters,
                     d_records->primal, d_records->dual, tol ? *tol : cert_default_tol(), d_residuals, d_verdict};
    return hmpc_launch_certify(h, a, stream);
}

extern "C" int hmpc_certify_batch(hmpc_handle *h, const double *x0, int32_t x0_stride, const int8_t *fix, int32_t B,
                                  const hmpc_result *records, const hmpc_cert_tol *tol, double *residuals, int32_t *verdict)
{
    g_err.clear();
    if (B < 0) return fail(HMPC_EINVAL, "bad batch size");
    if (h && B == 0) return HMPC_OK; // (an empty batch has no arrays to speak of: a view of an empty array may be null)
    int rc = certify_arguments(x0, x0_stride, B, records, residuals);
    if (rc) return rc;
    if (!h) return fail(HMPC_EINVAL, "null handle");
    if (!fix && h->cert.nub > 0) return fail(HMPC_EINVAL, "null argument");
    if (x0_stride != 0 && x0_stride < h->cert.nx) return fail(HMPC_EINVAL, "bad x0 stride");
    HIPCHK(hipSetDevice(h->device));
    const CertProb &c = h->cert;
    // the handle's two staging blocks (as the host-pointer solve uses them): inputs, then the two outputs
    const size_t n = (size_t)B, nfix = (size_t)c.T * c.nub;
    struct Part { size_t bytes; const void *src; size_t off; };
    Part parts[] = {{(x0_stride ? n : 1) * c.nx * sizeof(double), nullptr, 0}, {n * nfix, fix, 0}, {n * sizeof(double), records->obj, 0},
                    {n * sizeof(double), records->dual_obj, 0}, {n * sizeof(int32_t), records->status, 0}, {n * sizeof(int32_t), records->iters, 0},
                    {n * c.n_primal * sizeof(double), records->primal, 0}, {n * c.n_dual * sizeof(double), records->dual, 0},
                    {n * HMPC_CERT_COUNT * sizeof(double), nullptr, 0}, {n * sizeof(int32_t), nullptr, 0}};
    size_t total = 0;
    for (Part &q : parts) { q.off = total; total += (q.bytes + 255) / 256 * 256; }
    const size_t in_bytes = parts[8].off;
    HIPCHK(h->d_stage.grow(total, total, nullptr));
    HIPCHK(h->h_stage.grow(total, total, nullptr));
    char *hs = h->h_stage, *ds = h->d_stage;
    for (size_t b = 0; b < (x0_stride ? n : 1); b++)
        std::memcpy(hs + b * c.nx * sizeof(double), x0 + b * (size_t)x0_stride, c.nx * sizeof(double));
    for (const Part &q : parts)
        if (q.src && q.bytes) std::memcpy(hs + q.off, q.src, q.bytes);
    HIPCHK(hipMemcpyAsync(ds, hs, in_bytes, hipMemcpyHostToDevice, nullptr));
    const hmpc_result d{(double *)(ds + parts[2].off), (double *)(ds + parts[3].off), (int32_t *)(ds + parts[4].off),
                        (int32_t *)(ds + parts[5].off), (double *)(ds + parts[6].off), (double *)(ds + parts[7].off)};
    rc = hmpc_certify_batch_device(h, (const double *)ds, x0_stride ? c.nx : 0, (const int8_t *)(ds + parts[1].off), B, &d, tol,
                                   (double *)(ds + parts[8].off), (int32_t *)(ds + parts[9].off), nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(hs + in_bytes, ds + in_bytes, total - in_bytes, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    std::memcpy(residuals, hs + parts[8].off, parts[8].bytes);
    if (verdict) std::memcpy(verdict, hs + parts[9].off, parts[9].bytes);
    return HMPC_OK;
}

// ---- Branching a batch of solved nodes (include/hmpc.h; kernels: hmpc_branch.hip, arithmetic: hmpc_branch.h) -------------------
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

extern "C" int hmpc_branch_batch(hmpc_handle *h, const int8_t *fix, int32_t B, const hmpc_result *records, const double *cutoff,
                                 int32_t warm_base, int32_t mark_weak, const hmpc_branch_out *out)
{
    g_err.clear();
    if (B < 0) return fail(HMPC_EINVAL, "bad batch size");
    if (h && B == 0) return HMPC_OK;
    int rc = branch_arguments(h, fix, B, records, mark_weak, out);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const BranchDims d = branch_dims_of(h);
    const size_t n = (size_t)B, nfix = (size_t)d.nfix;
    const bool children = out->child_fix || out->child_lb || out->child_parent || out->child_warm;
    // the handle's two staging blocks (as the host-pointer solve uses them): inputs, then outputs; a part nobody asks for has no bytes
    enum { P_FIX, P_OBJ, P_STATUS, P_ITERS, P_PRIMAL, P_DUAL, P_CUTOFF, P_DOBJ, O_OBJ, O_WORD, O_POS, O_LB2, O_BITS, O_OFF, O_N, O_CFIX, O_CLB, O_CPAR, O_CWARM, PARTS };
    struct Part { size_t bytes; const void *src; void *dst; size_t off; };
    Part parts[PARTS] = {{n * nfix, fix, nullptr, 0},
                         {n * sizeof(double), records->obj, nullptr, 0},
                         {n * sizeof(int32_t), records->status, nullptr, 0},
                         {n * sizeof(int32_t), records->iters, nullptr, 0},
                         {out->bits ? n * d.n_primal * sizeof(double) : 0, records->primal, nullptr, 0},
                         {(out->child_lb2 || out->child_lb) ? n * d.n_dual * sizeof(double) : 0, records->dual, nullptr, 0},
                         {cutoff ? n * sizeof(double) : 0, cutoff, nullptr, 0},
                         {mark_weak ? n * sizeof(double) : 0, records->dual_obj, records->dual_obj, 0}, // (in and out: first of the outputs)
                         {out->obj ? n * sizeof(double) : 0, nullptr, out->obj, 0},
                         {out->word ? n * sizeof(int32_t) : 0, nullptr, out->word, 0},
                         {out->pos ? n * sizeof(int32_t) : 0, nullptr, out->pos, 0},
                         {out->child_lb2 ? 2 * n * sizeof(double) : 0, nullptr, out->child_lb2, 0},
                         {out->bits ? n * d.words * sizeof(uint64_t) : 0, nullptr, out->bits, 0},
                         {out->child_offset ? n * sizeof(int32_t) : 0, nullptr, out->child_offset, 0},
                         {(out->n_children || children) ? sizeof(int32_t) : 0, nullptr, out->n_children, 0}, // (the children are copied out up to it)
                         {out->child_fix ? 2 * n * nfix : 0, nullptr, out->child_fix, 0},
                         {out->child_lb ? 2 * n * sizeof(double) : 0, nullptr, out->child_lb, 0},
                         {out->child_parent ? 2 * n * sizeof(int32_t) : 0, nullptr, out->child_parent, 0},
                         {out->child_warm ? 2 * n * sizeof(int32_t) : 0, nullptr, out->child_warm, 0}};
    size_t total = 0;
    for (Part &q : parts) { q.off = total; total += (q.bytes + 255) / 256 * 256; }
    const size_t out_begin = parts[P_DOBJ].off;
    HIPCHK(h->d_stage.grow(total, total, nullptr));
    HIPCHK(h->h_stage.grow(total, total, nullptr));
    char *hs = h->h_stage, *ds = h->d_stage;
    for (int i = 0; i <= P_DOBJ; i++)
        if (parts[i].bytes) std::memcpy(hs + parts[i].off, parts[i].src, parts[i].bytes);
    HIPCHK(hipMemcpyAsync(ds, hs, parts[O_OBJ].off, hipMemcpyHostToDevice, nullptr));
    auto dev = [&](int i) -> char * { return parts[i].bytes ? ds + parts[i].off : nullptr; };
    const hmpc_result r{(double *)dev(P_OBJ), (double *)dev(P_DOBJ), (int32_t *)dev(P_STATUS), (int32_t *)dev(P_ITERS), (double *)dev(P_PRIMAL), (double *)dev(P_DUAL)};
    const hmpc_branch_out o{(double *)dev(O_OBJ), (int32_t *)dev(O_WORD), (int32_t *)dev(O_POS), (double *)dev(O_LB2), (uint64_t *)dev(O_BITS), (int32_t *)dev(O_OFF),
                            (int32_t *)dev(O_N), (int8_t *)dev(O_CFIX), (double *)dev(O_CLB), (int32_t *)dev(O_CPAR), (int32_t *)dev(O_CWARM)};
    rc = hmpc_branch_batch_device(h, (const int8_t *)ds, B, &r, (const double *)dev(P_CUTOFF), warm_base, mark_weak, &o, nullptr);
    if (rc) return rc;
    if (total > out_begin) HIPCHK(hipMemcpyAsync(hs + out_begin, ds + out_begin, total - out_begin, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    int32_t nchild = 0;
    if (parts[O_N].bytes) std::memcpy(&nchild, hs + parts[O_N].off, sizeof nchild);
    if (nchild < 0 || (size_t)nchild > 2 * n) return fail(HMPC_EDEVICE, "branch: the device returned a number of children outside [0, 2 B]");
    for (int i = P_DOBJ; i < PARTS; i++) {
        const Part &q = parts[i];
        if (!q.bytes || !q.dst) continue;
        // (rows of the child arrays at and beyond n_children are not written: neither on the device nor here)
        const size_t bytes = i >= O_CFIX ? q.bytes / (2 * n) * (size_t)nchild : q.bytes;
        std::memcpy(q.dst, hs + q.off, bytes);
    }
    return HMPC_OK;
}

// ---- K searches with their trees on the device (include/hmpc_search.h; kernels: hmpc_search.hip, arithmetic: hmpc_search.h) ----
struct hmpc_search {
    hmpc_handle *h = nullptr;
    BranchDims d{};
    SearchState v{};       // views into the blocks below
    DevBuf<int8_t> fix, b_fix;
    DevBuf<double> lb, td, x0, p_obj, p_dual_obj, p_primal, p_dual, b_x0;
    DevBuf<int32_t> row, wrow, ti, p_status, p_iters, picks, count, offset, word, b_idx;
    DevBuf<uint8_t> alive;
    DevBuf<char> tmp;      // begin's compact trees, the outputs of results and leaves
    PinBuf<int32_t> h_word;
    int32_t row0 = 0;      // first pool row of the staged (or next) round
    int32_t staged = 0;    // size of the staged round, 0: none
    bool begun = false;
};

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
    HIPCHK(s->p_dual_obj.alloc(rows));
    HIPCHK(s->p_status.alloc(rows));
    HIPCHK(s->p_iters.alloc(rows));
    HIPCHK(s->p_primal.alloc(rows * d.n_primal));
    HIPCHK(s->p_dual.alloc(rows * d.n_dual));
    HIPCHK(s->picks.alloc(k * SEARCH_MAX_WIDTH));
    HIPCHK(s->count.alloc(k));
    HIPCHK(s->offset.alloc(k));
    HIPCHK(s->word.alloc(4));
    HIPCHK(s->h_word.alloc(4));
    HIPCHK(s->b_fix.alloc(batch * d.nfix));
    HIPCHK(s->b_x0.alloc(batch * d.nx));
    HIPCHK(s->b_idx.alloc(3 * batch));
    int32_t *ti = s->ti;
    double *td = s->td;
    int32_t *bi = s->b_idx;
    s->v = SearchState{K, node_cap, row_cap, s->fix, s->lb, s->row, s->wrow, s->alive, ti, ti + k, ti + 2 * k, ti + 3 * k, ti + 4 * k, ti + 5 * k,
                       td, td + k, s->x0, s->p_obj, s->p_dual_obj, s->p_status, s->p_iters, s->p_primal, s->p_dual, s->picks, s->count, s->offset, s->word,
                       s->b_fix, s->b_x0, bi, bi + batch, bi + 2 * batch};
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
        const size_t o_fix = (K + 1) * sizeof(int32_t), o_lb = (o_fix + total * d.nfix + 7) / 8 * 8, bytes = o_lb + total * sizeof(double);
        HIPCHK(s->tmp.grow(bytes, bytes, nullptr));
        char *t = s->tmp;
        HIPCHK(hipMemcpy(t, off.data(), o_fix, hipMemcpyHostToDevice));
        if (total) {
            HIPCHK(hipMemcpy(t + o_fix, fix, total * d.nfix, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(t + o_lb, lb, total * sizeof(double), hipMemcpyHostToDevice));
            if (dual) {
                HIPCHK(hipMemcpy(s->p_dual, dual, total * d.n_dual * sizeof(double), hipMemcpyHostToDevice));
                HIPCHK(hipMemcpy(s->p_dual_obj, dual_obj, total * sizeof(double), hipMemcpyHostToDevice));
            }
        }
        g = SearchBegin{(const int32_t *)t, (const int8_t *)(t + o_fix), (const double *)(t + o_lb), dual != nullptr};
    }
    hipLaunchKernelGGL(hmpc_search_begin_kernel, search_grid((long long)K), dim3(64 * SEARCH_WAVES), 0, nullptr, d, s->v, g);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));
    s->row0 = dual ? (int32_t)total : 0;
    s->staged = 0;
    s->begun = true;
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
    s->staged = 0;
    hipLaunchKernelGGL(hmpc_search_select_kernel, dim3(s->v.K), dim3(SEARCH_SELECT_THREADS), 0, st, s->d, s->v, (int)width, tol);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hmpc_search_offsets_kernel, dim3(1), dim3(SEARCH_SCAN_CHUNK), 0, st, s->d, s->v, (int)s->row0, hd);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(hmpc_search_stage_kernel, search_grid((long long)s->v.K * width), dim3(64 * SEARCH_WAVES), 0, st, s->d, s->v, (int)width, hd);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->h_word, s->word, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int32_t *w = s->h_word;
    if (w[0] < 0 || (long long)w[0] > (long long)s->v.K * width) return fail(HMPC_EDEVICE, "search: the device returned a round size outside [0, K width]");
    *B = w[0];
    if (!w[3]) return fail(HMPC_ETOOBIG, "search: the round's records do not fit the pool (row_cap)");
    s->staged = w[0];
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
    if (s->staged <= 0) return fail(HMPC_EINVAL, "search: no round is staged (hmpc_search_select)");
    HIPCHK(hipSetDevice(s->h->device));
    hipLaunchKernelGGL(hmpc_search_consume_kernel, search_grid((long long)s->v.K), dim3(64 * SEARCH_WAVES), 0, (hipStream_t)stream, s->d, s->v, (int)s->row0, tol);
    HIPCHK(hipGetLastError());
    s->row0 += s->staged;
    s->staged = 0;
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
        if (B == 0) break;
        const double *x0;
        const int8_t *fix;
        hmpc_warm warm;
        hmpc_result rows;
        hmpc_search_batch(s, &x0, &fix, &warm, &rows, nullptr);
        // (as the host-pointer solve does: the hand-down kernel only where a node of the round receives a record)
        if ((rc = hmpc_solve_batch_device(s->h, x0, s->d.nx, fix, B, s->h_word[2] ? &warm : nullptr, &rows, stream))) return rc;
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
    struct Part { size_t bytes; void *dst; size_t off; };
    Part parts[8] = {{cost ? K * sizeof(double) : 0, cost, 0},           {u0 ? K * d.nu * sizeof(double) : 0, u0, 0},
                     {x1 ? K * d.nx * sizeof(double) : 0, x1, 0},       {solves ? K * sizeof(int32_t) : 0, solves, 0},
                     {leaves ? K * sizeof(int32_t) : 0, leaves, 0},     {state ? K * sizeof(int32_t) : 0, state, 0},
                     {uncertified ? K * sizeof(int32_t) : 0, uncertified, 0}, {binaries ? K * d.nfix : 0, binaries, 0}};
    size_t total = 0;
    for (Part &q : parts) { q.off = total; total += (q.bytes + 255) / 256 * 256; }
    if (!total) return HMPC_OK;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(s->tmp.grow(total, total, nullptr));
    char *t = s->tmp;
    auto dev = [&](int i) -> char * { return parts[i].bytes ? t + parts[i].off : nullptr; };
    const SearchResults r{(double *)dev(0), (double *)dev(1), (double *)dev(2), (int8_t *)dev(7), (int32_t *)dev(3), (int32_t *)dev(4), (int32_t *)dev(5), (int32_t *)dev(6)};
    hipLaunchKernelGGL(hmpc_search_results_kernel, search_grid((long long)K), dim3(64 * SEARCH_WAVES), 0, nullptr, d, s->v, r);
    HIPCHK(hipGetLastError());
    for (const Part &q : parts)
        if (q.bytes) HIPCHK(hipMemcpy(q.dst, t + q.off, q.bytes, hipMemcpyDeviceToHost));
    return HMPC_OK;
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
    const size_t N = (size_t)total;
    struct Part { size_t bytes; void *dst; size_t off; };
    Part parts[7] = {{K * sizeof(int32_t), nullptr, 0},
                     {owner ? N * sizeof(int32_t) : 0, owner, 0},
                     {lb ? N * sizeof(double) : 0, lb, 0},
                     {dual_obj ? N * sizeof(double) : 0, dual_obj, 0},
                     {dual ? N * d.n_dual * sizeof(double) : 0, dual, 0},
                     {fix ? N * d.nfix : 0, fix, 0},
                     {has_dual ? N : 0, has_dual, 0}};
    size_t bytes = 0;
    for (Part &q : parts) { q.off = bytes; bytes += (q.bytes + 255) / 256 * 256; }
    HIPCHK(s->tmp.grow(bytes, bytes, nullptr));
    char *t = s->tmp;
    auto dev = [&](int i) -> char * { return parts[i].bytes ? t + parts[i].off : nullptr; };
    HIPCHK(hipMemcpy(t, off.data(), K * sizeof(int32_t), hipMemcpyHostToDevice));
    const SearchLeaves o{(const int32_t *)t, (int32_t *)dev(1), (int8_t *)dev(5), (double *)dev(2), (double *)dev(4), (double *)dev(3), (uint8_t *)dev(6)};
    hipLaunchKernelGGL(hmpc_search_leaves_kernel, search_grid((long long)K), dim3(64 * SEARCH_WAVES), 0, nullptr, d, s->v, o);
    HIPCHK(hipGetLastError());
    for (int i = 1; i < 7; i++)
        if (parts[i].bytes) HIPCHK(hipMemcpy(parts[i].dst, t + parts[i].off, parts[i].bytes, hipMemcpyDeviceToHost));
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
    struct Part { void *host, *dev; size_t bytes; };
    const Part parts[6] = {{host->obj, v.p_obj + r, n * sizeof(double)},
                           {host->dual_obj, v.p_dual_obj + r, n * sizeof(double)},
                           {host->status, v.p_status + r, n * sizeof(int32_t)},
                           {host->iters, v.p_iters + r, n * sizeof(int32_t)},
                           {host->primal, v.p_primal + r * d.n_primal, n * d.n_primal * sizeof(double)},
                           {host->dual, v.p_dual + r * d.n_dual, n * d.n_dual * sizeof(double)}};
    for (const Part &q : parts) {
        if (!q.host || !q.bytes) continue;
        if (write) HIPCHK(hipMemcpy(q.dev, q.host, q.bytes, hipMemcpyHostToDevice));
        else HIPCHK(hipMemcpy(q.host, q.dev, q.bytes, hipMemcpyDeviceToHost));
    }
    return HMPC_OK;
}

#include "hmpc_fleet.hip" // closed loops in lockstep (same translation unit: uses the launchers above)
#include "hmpc_comm.hip"  // incumbent all-reduce over RCCL
#include "hmpc_lp.hip"    // batched dense LPs of the offline terminal ingredients
