// hmpc_certify.hip -- KKT / Farkas certificate of a batch of QP records on the device (hmpc_certify_batch, include/hmpc.h).
//
// One wavefront per record, several records per workgroup, persistent over the batch: the shape of the shift kernel
// (hmpc_shift.hip).  What a record's certificate IS lives in hmpc_certify.h, item by item, and compiles for the host as well;
// this file supplies the lane loop (cert_accumulate with first = lane, step = 64: lanes stride over the flat item lists -- dual
// entries, stationarity entries, dynamics entries, inequality and bound rows, objective terms), the wave reductions in f64
// (NaN-propagating maxima, sums) and the staging.
//
// Memory: a record is read once -- one primal and one dual row, ~10 KB on the cart-pole at N = 20 -- and ten doubles and a
// word are written; every item is a short dot product of a row segment with a row or column of one of the problem's
// matrices.  So the rows of a wave's record are copied to LDS once (coalesced 8-byte loads: n_dual is odd for some problems,
// a row has no 16-byte alignment) and the matrices once per workgroup, and the items read LDS only.  Three forms, chosen by
// the host from the sizes (hmpc_launch_certify):
//   <matrices in LDS, rows in LDS>  as many waves per workgroup as LDS has room for rows (4 .. 16), one workgroup per CU
//   <matrices in LDS, rows global>  rows that leave room for fewer than four waves (configs[4]: 44 KB per record) stay in
//                                   global memory: their re-reads by the lanes of the wave are L1 / L2 hits
//   <matrices global, rows global>  matrices beyond 64 KB are read in place too: no size limit
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hmpc_certify.h"
#include "hmpc_host.h" // the entries at the end of this file: hmpc_handle, the staging table and its transfers

#define CERT_WAVES 4       // waves per workgroup of the forms that read rows in place
#define CERT_MAX_WAVES 16  // ... of the form with rows in LDS (one workgroup per CU)

struct CertArgs {
    int B, x0_stride;
    const double *x0;
    const int8_t *fix;
    const double *obj, *dobj;
    const int32_t *status, *iters;
    const double *primal, *dual;
    hmpc_cert_tol tol;
    double *res;       // B x HMPC_CERT_COUNT
    int32_t *verdict;  // B, or null
};

static __device__ __forceinline__ double cert_wave_count(double v) // (small integers: exact)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the lanes' compensated partial sums into one, still compensated (cert_sum_merge is symmetric: every lane ends with the same bits)
static __device__ __forceinline__ CertSum cert_wave_sum(CertSum v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const CertSum other = {__shfl_xor(v.s, o), __shfl_xor(v.c, o)};
        cert_sum_merge(v, other);
    }
    return v;
}

static __device__ __forceinline__ double cert_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = cert_max(v, __shfl_xor(v, o));
    return v;
}

// doubles per wave of the row buffers: primal row, dual row, x0
static __host__ __device__ inline size_t hmpc_certify_row_doubles(const CertProb &p) { return (size_t)p.n_primal + p.n_dual + p.nx; }

template <bool MATS, bool ROWS>
__global__ void __launch_bounds__(64 * CERT_MAX_WAVES) hmpc_certify_kernel(const CertProb pg, const CertArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = blockDim.x >> 6;
    CertProb p = pg;
    size_t used = 0;
    if (MATS) {
        const size_t nm = cert_matrix_doubles(pg);
        for (size_t i = tid; i < nm; i += blockDim.x) sm[i] = pg.A[i]; // (one block, A first: cert_set_matrices)
        cert_set_matrices(p, sm);
        used = nm;
        __syncthreads();
    }
    double *rows = sm + used + (size_t)wave * hmpc_certify_row_doubles(pg);
    const int nfix = p.T * p.nub;
    for (int b = blockIdx.x * W + wave; b < a.B; b += gridDim.x * W) {
        const int status = a.status[b], cls = cert_class(status, a.iters[b]);
        double *out = a.res + (size_t)b * HMPC_CERT_COUNT;
        if (cls == HMPC_CERT_CLASS_SKIPPED) { // not decided: nothing of its rows is read
            if (lane < HMPC_CERT_COUNT) out[lane] = NAN;
            if (lane == 0 && a.verdict) a.verdict[b] = cls;
            continue;
        }
        const double *w = a.primal + (size_t)b * p.n_primal, *d = a.dual + (size_t)b * p.n_dual;
        const double *x0 = a.x0 + (size_t)b * a.x0_stride;
        const int8_t *fix = a.fix + (size_t)b * nfix;
        if (ROWS) {
            double *ws = rows, *ds = ws + p.n_primal, *xs = ds + p.n_dual;
            for (int i = lane; i < p.n_primal; i += 64) ws[i] = w[i];
            for (int i = lane; i < p.n_dual; i += 64) ds[i] = d[i];
            for (int i = lane; i < p.nx; i += 64) xs[i] = x0[i];
            w = ws; d = ds; x0 = xs;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier(); // the rows this wave wrote are read by all its lanes
        }
        CertAcc acc;
        cert_clear(acc);
        cert_accumulate(p, status, w, d, x0, fix, lane, 64, acc);
        acc.max_lam = cert_wave_max(acc.max_lam); acc.max_mu = cert_wave_max(acc.max_mu);
        acc.max_rho = cert_wave_max(acc.max_rho); acc.max_sig = cert_wave_max(acc.max_sig);
        acc.stat = cert_wave_max(acc.stat); acc.neg = cert_wave_max(acc.neg);
        acc.dobj = cert_wave_sum(acc.dobj);
        if (status == HMPC_INFEASIBLE) {
            acc.count = cert_wave_count(acc.count);
        } else {
            acc.peq = cert_wave_max(acc.peq); acc.pineq = cert_wave_max(acc.pineq);
            acc.pobj = cert_wave_sum(acc.pobj);
        }
        double res[HMPC_CERT_COUNT];
        cert_residuals(acc, status, a.obj[b], a.dobj[b], res); // (every lane holds the reduced values: every lane the same residuals)
        double mine = NAN;
#pragma unroll
        for (int c = 0; c < HMPC_CERT_COUNT; c++) mine = lane == c ? res[c] : mine;
        if (lane < HMPC_CERT_COUNT) out[lane] = mine;
        if (lane == 0 && a.verdict) a.verdict[b] = cert_verdict(cls, res, a.tol);
        if (ROWS) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier(); // the next record overwrites the buffers
        }
    }
}

// ---- Host side: the entries of include/hmpc.h (arithmetic: hmpc_certify.h) -----------------------------------------------------
// everything that can be said about the arguments without the device (after the batch size, which decides whether they are looked at)
static int certify_arguments(const hmpc_handle *h, const void *x0, int32_t x0_stride, const void *fix, const hmpc_result *r, const double *residuals)
{
    if (!x0 || !r || !residuals || !r->obj || !r->dual_obj || !r->status || !r->iters || !r->primal || !r->dual)
        return fail(HMPC_EINVAL, "null argument (all six members of the records are required)");
    if (x0_stride < 0) return fail(HMPC_EINVAL, "bad x0 stride");
    if (!h) return fail(HMPC_EINVAL, "null handle");
    if (!fix && h->cert.nub > 0) return fail(HMPC_EINVAL, "null argument");
    if (x0_stride != 0 && x0_stride < h->cert.nx) return fail(HMPC_EINVAL, "bad x0 stride");
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
    const size_t room = LDS_PER_CU, mats_most = 64 * 1024, mats = cert_matrix_doubles(c) * sizeof(double), per = hmpc_certify_row_doubles(c) * sizeof(double);
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
    const int rc = certify_arguments(h, d_x0, x0_stride, d_fix, d_records, d_residuals);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const CertArgs a{B, x0_stride, d_x0, d_fix, d_records->obj, d_records->dual_obj, d_records->status, d_records->iters,
                     d_records->primal, d_records->dual, tol ? *tol : cert_default_tol(), d_residuals, d_verdict};
    return hmpc_launch_certify(h, a, stream);
}

// the handle's two staging blocks (as the host-pointer solve uses them, exact fit): the inputs up, the two outputs down
extern "C" int hmpc_certify_batch(hmpc_handle *h, const double *x0, int32_t x0_stride, const int8_t *fix, int32_t B,
                                  const hmpc_result *records, const hmpc_cert_tol *tol, double *residuals, int32_t *verdict)
{
    g_err.clear();
    if (B < 0) return fail(HMPC_EINVAL, "bad batch size");
    if (h && B == 0) return HMPC_OK; // (an empty batch has no arrays to speak of: a view of an empty array may be null)
    int rc = certify_arguments(h, x0, x0_stride, fix, records, residuals);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const StageTable t = stage_certify(stage_dims(h), (size_t)B, x0, (size_t)x0_stride, fix, *records, residuals, verdict);
    if ((rc = stage_room(h, t.total, t.total)) || (rc = stage_up(h, t))) return rc;
    char *ds = h->d_stage;
    const CertArgs a{B, x0_stride ? h->cert.nx : 0, t.ptr<double>(CERT_X0, ds), t.ptr<int8_t>(CERT_FIX, ds), t.ptr<double>(CERT_OBJ, ds),
                     t.ptr<double>(CERT_DOBJ, ds), t.ptr<int32_t>(CERT_STATUS, ds), t.ptr<int32_t>(CERT_ITERS, ds), t.ptr<double>(CERT_PRIMAL, ds),
                     t.ptr<double>(CERT_DUAL, ds), tol ? *tol : cert_default_tol(), t.ptr<double>(CERT_RES, ds), t.ptr<int32_t>(CERT_VERDICT, ds)};
    if ((rc = hmpc_launch_certify(h, a, nullptr)) || (rc = stage_down(h, t, t.total))) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    t.unpack(h->h_stage, CERT_RES);
    t.unpack(h->h_stage, CERT_VERDICT);
    return HMPC_OK;
}
