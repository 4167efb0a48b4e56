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
#include "hmpc_host.h"     // error text, Buffer, hmpc_handle, the transfers of a staging table
// each family's kernels with its entries (as hmpc_fleet.hip, hmpc_comm.hip and hmpc_lp.hip at the end of this file)
#include "hmpc_shift.hip"   // the warm-start node shift (hmpc_set_shift_maps, hmpc_shift_batch)
#include "hmpc_certify.hip" // certificates of a batch of records (hmpc_certify_batch)
#include "hmpc_branch.hip"  // branching a batch of solved nodes (hmpc_branch_batch)
#include "hmpc_search.hip"  // the rounds of K device-resident searches (include/hmpc_search.h)

#define HMPC_CHECK_NODES 64 // (even) nodes of the first-use check of a kernel compiled at hmpc_create (hmpc_check_compiled)

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
    if (const char *e = getenv("HMPC_WAVES")) { const int nw = atoi(e); only = nw == 1 || nw == 2 || nw == 4 ? hmpc_cfg_index(nw) : -1; }
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

// what can be said about the arguments of a solve before the batch size decides whether anything is done (the hand-down is looked at after it)
static int solve_arguments(const hmpc_handle *h, const double *x0, int32_t x0_stride, const int8_t *fix, int32_t B, const hmpc_result *out)
{
    if (!h || !x0 || !fix || !out) return fail(HMPC_EINVAL, "null argument");
    if (B < 0 || (x0_stride != 0 && x0_stride < h->dp.nx)) return fail(HMPC_EINVAL, "bad batch size or x0 stride");
    return HMPC_OK;
}
static bool warm_without_rows(const hmpc_warm *w) { return w && w->index && (!w->primal || !w->dual); }

extern "C" int hmpc_solve_batch_device(hmpc_handle *h, const double *d_x0, int32_t x0_stride, const int8_t *d_fix,
                                       int32_t B, const hmpc_warm *d_warm, const hmpc_result *d_out, void *stream)
{
    g_err.clear();
    const int rc0 = solve_arguments(h, d_x0, x0_stride, d_fix, B, d_out);
    if (rc0) return rc0;
    if (B == 0) return HMPC_OK;
    HIPCHK(hipSetDevice(h->device));
    hmpc_second_opinion_review_impl(h, false);
    if (warm_without_rows(d_warm)) return fail(HMPC_EINVAL, "hmpc_warm: index without record rows");
    DevOut o{d_out->obj, d_out->dual_obj, d_out->status, d_out->iters, d_out->primal, d_out->dual};
    DevWarm w{nullptr, nullptr, nullptr, nullptr, 0};
    if (d_warm && d_warm->index) w = DevWarm{d_warm->primal, d_warm->dual, d_warm->index, nullptr, 0};
    int nw = hmpc_waves_for(B, h->cfg[0].max_grid);
    // the streaming form holds one node per CU whatever the number of waves: always spread it over all four SIMDs
    if (h->cfg[2].k.big && !getenv("HMPC_WAVES")) nw = 4;
    h->last_cfg = hmpc_cfg_index(nw);
    hmpc_cfg &cfm = h->cfg[h->last_cfg];
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
// the order obj | dual_obj | status | iters | primal | dual (hmpc_stage.h: stage_solve) -- one copy up, one copy down per call
// (round 1: two pageable copies up, six down, each its own synchronisation: ~100 us of a 1.4 ms branch-and-bound round).
// Room in both blocks for a batch of B nodes, nw of them with a parent record; a block that is short is replaced by one
// for 64 nodes, or B + B / 4 from 64 on (each with room for a record if any of this batch has one)
static int ensure_staging(hmpc_handle *h, size_t B, size_t nw)
{
    const size_t cap = B < 64 ? 64 : B + B / 4;
    const StageDims d = stage_dims(h);
    return stage_room(h, stage_solve(d, B, nw, nullptr, 0, nullptr, nullptr).total, stage_solve(d, cap, nw ? cap : 0, nullptr, 0, nullptr, nullptr).total);
}

extern "C" int hmpc_solve_batch(hmpc_handle *h, const double *x0, int32_t x0_stride, const int8_t *fix, int32_t B,
                                const hmpc_warm *warm, const hmpc_result *out)
{
    g_err.clear();
    int rc = solve_arguments(h, x0, x0_stride, fix, B, out);
    if (rc) return rc;
    if (B == 0) return HMPC_OK;
    HIPCHK(hipSetDevice(h->device));
    const DevProb &p = h->dp;
    // parent records handed down: gathered, one row per node that has one (the index is rewritten to the gathered rows)
    size_t nwarm = 0;
    if (warm_without_rows(warm)) return fail(HMPC_EINVAL, "hmpc_warm: index without record rows");
    if (warm && warm->index)
        for (int b = 0; b < B; b++) {
            if (warm->index[b] >= warm->rows) return fail(HMPC_EINVAL, "hmpc_warm: index beyond the rows handed in");
            nwarm += warm->index[b] >= 0;
        }
    if ((rc = ensure_staging(h, (size_t)B, nwarm))) return rc;
    // offsets of THIS batch (they always fit the capacity the blocks were allocated for): with the capacity's offsets
    // a small branch-and-bound round after one large call dragged the whole capacity-sized primal region along
    const StageTable t = stage_solve(stage_dims(h), (size_t)B, nwarm, x0, (size_t)x0_stride, fix, out);
    char *hs = h->h_stage, *ds = h->d_stage;
    hmpc_warm dw{nullptr, nullptr, nullptr, 0};
    if (nwarm) {
        int32_t *idx = t.ptr<int32_t>(SOLVE_WIDX, hs);
        double *wp = t.ptr<double>(SOLVE_WPRIMAL, hs), *wd = t.ptr<double>(SOLVE_WDUAL, hs);
        size_t q = 0;
        for (int b = 0; b < B; b++) {
            const int32_t r = warm->index[b];
            idx[b] = r >= 0 ? (int32_t)q : -1;
            if (r < 0) continue;
            std::memcpy(wp + q * p.n_primal, warm->primal + (size_t)r * p.n_primal, p.n_primal * sizeof(double));
            std::memcpy(wd + q * p.n_dual, warm->dual + (size_t)r * p.n_dual, p.n_dual * sizeof(double));
            q++;
        }
        dw = hmpc_warm{t.ptr<double>(SOLVE_WPRIMAL, ds), t.ptr<double>(SOLVE_WDUAL, ds), t.ptr<int32_t>(SOLVE_WIDX, ds), (int32_t)nwarm};
    }
    if ((rc = stage_up(h, t))) return rc;
    const hmpc_result d{t.ptr<double>(SOLVE_OBJ, ds), t.ptr<double>(SOLVE_DOBJ, ds), t.ptr<int32_t>(SOLVE_STATUS, ds), t.ptr<int32_t>(SOLVE_ITERS, ds),
                        t.ptr<double>(SOLVE_PRIMAL, ds), t.ptr<double>(SOLVE_DUAL, ds)};
    rc = hmpc_solve_batch_device(h, t.ptr<double>(SOLVE_X0, ds), x0_stride == 0 ? 0 : p.nx, t.at<int8_t>(SOLVE_FIX, ds), B,
                                 nwarm ? &dw : nullptr, &d, nullptr);
    if (rc) return rc;
    // small outputs in one copy through the pinned block; large primal / dual blocks straight into the caller's arrays
    // (a pageable copy is pipelined by the runtime, a detour through the staging block would not be)
    const StagePart &pr = t.part[SOLVE_PRIMAL], &du = t.part[SOLVE_DUAL];
    const bool big = (size_t)B * (p.n_primal + p.n_dual) * sizeof(double) > (size_t)4 << 20;
    if ((rc = stage_down(h, t, big ? pr.off : du.bytes ? t.end(SOLVE_DUAL) : t.end(SOLVE_PRIMAL)))) return rc;
    if (big) {
        if (pr.bytes) HIPCHK(hipMemcpyAsync(pr.dst, ds + pr.off, pr.bytes, hipMemcpyDeviceToHost, nullptr));
        if (du.bytes) HIPCHK(hipMemcpyAsync(du.dst, ds + du.off, du.bytes, hipMemcpyDeviceToHost, nullptr));
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
    for (int i = SOLVE_OBJ; i <= (big ? SOLVE_ITERS : SOLVE_DUAL); i++) t.unpack(hs, i);
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


#include "hmpc_fleet.hip" // closed loops in lockstep (same translation unit: uses the launchers above)
#include "hmpc_comm.hip"  // incumbent all-reduce over RCCL
#include "hmpc_lp.hip"    // batched dense LPs of the offline terminal ingredients
