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
