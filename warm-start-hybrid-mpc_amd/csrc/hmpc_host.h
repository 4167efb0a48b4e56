// hmpc_host.h -- what the host side of every entry family shares: the error text, the owner of device and pinned memory, the
// handle, and the transfers of a staging table (hmpc_stage.h).  Part of the launching translation unit (hmpc_capi.hip), after
// hmpc_kernel.hip: the family files (hmpc_shift.hip, hmpc_certify.hip, hmpc_branch.hip, hmpc_search.hip, hmpc_fleet.hip ...)
// hold their kernels and their extern "C" entries together and are included there.
#ifndef HMPC_HOST_H
#define HMPC_HOST_H

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "hmpc_device.h"
#include "hmpc_certify.h" // CertProb
#include "hmpc_stage.h"

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
    DevBuf<char> d_stage; // one device block (inputs, then outputs: hmpc_stage.h)
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

constexpr size_t LDS_PER_CU = 160 * 1024;

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

// configuration (hmpc_handle::cfg) of a wave count per node: 1, 2, 4 -> 0, 1, 2
static inline int hmpc_cfg_index(int nw) { return nw == 1 ? 0 : nw == 2 ? 1 : 2; }

// ---- Transfers of a staging table (hmpc_stage.h) ------------------------------------------------------------------------------
static StageDims stage_dims(const hmpc_handle *h)
{
    const DevProb &p = h->dp;
    const size_t nfix = (size_t)p.T * p.nub;
    return StageDims{(size_t)p.nx, (size_t)p.nu, nfix, (nfix + 63) / 64, (size_t)p.n_primal, (size_t)p.n_dual};
}
// Room for `want` bytes in the handle's staging block and its pinned mirror; a block that is short is replaced by one of `cap` bytes
static int stage_room(hmpc_handle *h, size_t want, size_t cap)
{
    HIPCHK(h->d_stage.grow(want, cap, nullptr));
    HIPCHK(h->h_stage.grow(want, cap, nullptr));
    return HMPC_OK;
}
// The table's sources into the pinned block, then ONE copy up; ONE copy down of the outputs up to `end` (null stream, not waited for)
static int stage_up(hmpc_handle *h, const StageTable &t)
{
    t.pack(h->h_stage);
    HIPCHK(hipMemcpyAsync(h->d_stage, h->h_stage, t.in_end, hipMemcpyHostToDevice, nullptr));
    return HMPC_OK;
}
static int stage_down(hmpc_handle *h, const StageTable &t, size_t end)
{
    const size_t o = t.out_begin;
    if (end > o) HIPCHK(hipMemcpyAsync(h->h_stage + o, h->d_stage + o, end - o, hipMemcpyDeviceToHost, nullptr));
    return HMPC_OK;
}
// Without a pinned mirror: one copy per present part between the caller's own arrays and the device block `base`, on the null
// stream and not waited for (async), or blocking -- the inputs up, the outputs down
static int stage_each_up(const StageTable &t, char *base, bool async)
{
    for (int i = 0; i < t.n_in; i++) {
        const StagePart &p = t.part[i];
        if (!p.bytes || !p.src) continue;
        HIPCHK(async ? hipMemcpyAsync(base + p.off, p.src, p.bytes, hipMemcpyHostToDevice, nullptr) : hipMemcpy(base + p.off, p.src, p.bytes, hipMemcpyHostToDevice));
    }
    return HMPC_OK;
}
static int stage_each_down(const StageTable &t, const char *base, bool async)
{
    for (int i = t.n_in; i < t.n; i++) {
        const StagePart &p = t.part[i];
        if (!p.bytes || !p.dst) continue;
        HIPCHK(async ? hipMemcpyAsync(p.dst, base + p.off, p.bytes, hipMemcpyDeviceToHost, nullptr) : hipMemcpy(p.dst, base + p.off, p.bytes, hipMemcpyDeviceToHost));
    }
    return HMPC_OK;
}

#endif
