// certify_driver.cpp -- the CPU form of hmpc_certify_batch: a serial loop over the per-item functions of csrc/hmpc_certify.h
// (one "lane" takes every item), built with -fsanitize=address,undefined by tests/test_certify_host.py.  It restates none of
// the arithmetic: problem, records and tolerances in from a file, residuals and verdicts out to another.
//
//   certify_driver <in> <out>
//   in : int32 nx nu nub T nc ncT nq nr nqT B x0_stride has_tol | float64 A B F G h F_Tm1 G_Tm1 h_Tm1 Q R Q_T (row-major)
//        | float64 tol[4] | float64 x0 (nx, or B x nx) | int8 fix (B x T nub) | float64 obj[B] dual_obj[B] | int32 status[B] iters[B]
//        | float64 primal (B x n_primal) dual (B x n_dual)
//   out: float64 residuals (B x HMPC_CERT_COUNT) | int32 verdict[B]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hmpc_certify.h"

template <class T> static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "certify_driver: input too short\n");
        exit(2);
    }
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    if (!cert_sum_self_test()) { // (a build that contracts or reassociates the compensated sums is not the arithmetic under test)
        fprintf(stderr, "certify_driver: the compensated sums of hmpc_certify.h do not hold in this build\n");
        return 3;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> n = take<int32_t>(f, 12);
    CertProb p{};
    cert_set_sizes(p, n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8]);
    const size_t B = (size_t)n[9], stride = (size_t)n[10];
    // every array in a block of its own, exactly as long as the layout says: an index beyond a row is a sanitizer report
    const std::vector<double> mats = take<double>(f, cert_matrix_doubles(p));
    cert_set_matrices(p, mats.data());
    const std::vector<double> tolv = take<double>(f, 4);
    hmpc_cert_tol tol = cert_default_tol();
    if (n[11]) { tol.polished = tolv[0]; tol.unpolished = tolv[1]; tol.infeasible = tolv[2]; tol.weak = tolv[3]; }
    const std::vector<double> x0 = take<double>(f, (stride ? B : 1) * p.nx);
    const size_t nfix = (size_t)p.T * p.nub;
    const std::vector<int8_t> fix = take<int8_t>(f, B * nfix);
    const std::vector<double> obj = take<double>(f, B), dobj = take<double>(f, B);
    const std::vector<int32_t> status = take<int32_t>(f, B), iters = take<int32_t>(f, B);
    std::vector<std::vector<double>> primal, dual;
    for (size_t b = 0; b < B; b++) primal.push_back(take<double>(f, p.n_primal));
    for (size_t b = 0; b < B; b++) dual.push_back(take<double>(f, p.n_dual));
    fclose(f);
    std::vector<double> res(B * HMPC_CERT_COUNT);
    std::vector<int32_t> verdict(B);
    for (size_t b = 0; b < B; b++) {
        const std::vector<int8_t> fb(fix.begin() + b * nfix, fix.begin() + (b + 1) * nfix);
        const std::vector<double> xb(x0.begin() + b * stride, x0.begin() + b * stride + p.nx);
        cert_record_serial(p, status[b], iters[b], obj[b], dobj[b], primal[b].data(), dual[b].data(), xb.data(), fb.data(), tol,
                           &res[b * HMPC_CERT_COUNT], &verdict[b]);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(res.data(), sizeof(double), res.size(), o);
    fwrite(verdict.data(), sizeof(int32_t), verdict.size(), o);
    fclose(o);
    return 0;
}
