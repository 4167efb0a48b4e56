// tree_driver.cpp -- host-only driver of the fleet's host logic (csrc/hmpc_tree.h) for AddressSanitizer / UBSan.
//
// TEST INFRASTRUCTURE (built and run by tests/test_sanitizers.py with g++ -fsanitize=address,undefined; the GPU pool has
// no device sanitizer).  It calls the functions hmpc_fleet_solve / hmpc_fleet_shift call, in their order --
// select, count and fill a round, record its results, consume, incumbent rows, close the step, retain, stage and adopt the
// shift -- on K trees, and stands in for the device only: the QP relaxations of every round are solved by the CPU oracle
// (liboracle_qp.so, loaded at run time) in place of the kernel launch, the row pools are host vectors, and the oracle's
// `polished` word becomes the C ABI's `iters` word, so that weak and uncertified nodes reach the code as they reach the
// library's.  It prints per step and tree the cost, the number of solves and of leaves as one JSON line; the Python test
// compares them with the Python branch and bound.
// The node shift itself is a device kernel and not part of this driver: the leaves a step retains are adopted with the
// bound -inf and flags 3 (every leaf kept and reopened -- a valid warm start whatever the model error), which drives the
// adoption and a warm-started search of the next step through the same code.
//
//   tree_driver PROBLEM.bin LIBORACLE K STEPS WIDTH SPECULATION DIVE HANDDOWN
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>

#include "hmpc_tree.h"

typedef int (*oracle_fn)(int, int, int, int, int, int, int, int, int, const double *, const double *, const double *, const double *, const double *,
                         const double *, const double *, const double *, const double *, const double *, const double *, const double *, int, int,
                         const int8_t *, double, double, int, int, int, int, int, double, const double *, const double *, const int32_t *, double *,
                         double *, int *, int *, double *, double *, int *);

static std::vector<double> read_block(FILE *f, size_t n)
{
    std::vector<double> v(n);
    if (n && fread(v.data(), sizeof(double), n, f) != n) { fprintf(stderr, "short problem file\n"); exit(2); }
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 9) { fprintf(stderr, "usage: tree_driver PROBLEM.bin LIBORACLE K STEPS WIDTH SPECULATION DIVE HANDDOWN\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror("problem file"); return 2; }
    int32_t dims[9]; // nx nu nub T nc ncL nq nr nqT
    if (fread(dims, sizeof(int32_t), 9, f) != 9) return 2;
    const int nx = dims[0], nu = dims[1], nub = dims[2], T = dims[3], nc = dims[4], ncL = dims[5], nq = dims[6], nr = dims[7], nqT = dims[8];
    const FleetDims d = fleet_dims(nx, nu, nub, T, nc, ncL, nq, nr, nqT);
    auto A = read_block(f, (size_t)nx * nx), Bm = read_block(f, (size_t)nx * nu), F = read_block(f, (size_t)nc * nx), G = read_block(f, (size_t)nc * nu),
         h = read_block(f, nc), FT = read_block(f, (size_t)ncL * nx), GT = read_block(f, (size_t)ncL * nu), hT = read_block(f, ncL),
         Q = read_block(f, (size_t)nq * nx), R = read_block(f, (size_t)nr * nu), QT = read_block(f, (size_t)nqT * nx);
    const int K = atoi(argv[3]), steps = atoi(argv[4]), width = atoi(argv[5]);
    FleetExpansion ex{atoi(argv[6]), atoi(argv[7]) != 0, atoi(argv[8]) != 0, {}, {}};
    auto x0s = read_block(f, (size_t)K * nx);
    fclose(f);
    void *lib = dlopen(argv[2], RTLD_NOW);
    if (!lib) { fprintf(stderr, "cannot load %s: %s\n", argv[2], dlerror()); return 2; }
    oracle_fn solve = (oracle_fn)dlsym(lib, "oracle_solve_batch");
    if (!solve) { fprintf(stderr, "oracle_solve_batch not found\n"); return 2; }
    const double inf = std::numeric_limits<double>::infinity();
    // the oracle's `polished` word (oracle/hsde_qp.c, oracle/oracle_qp.py) as the flags of hmpc_result.iters
    auto abi_iters = [](int polished) {
        return ((polished & 0xff) ? HMPC_ITERS_POLISHED : 0) | ((polished & 0x100) ? HMPC_ITERS_WEAK : 0) | ((polished & 0x400) ? HMPC_ITERS_UNCERTIFIED : 0);
    };
    std::vector<FleetTree> trees(K);
    for (auto &t : trees) tree_reset_cold(t, d.nfix);
    std::vector<double> pool_dual, pool_primal; // the row pools of a step (host copies of what lives in HBM)
    std::vector<std::vector<int>> picks(K), keep(K);
    std::vector<FleetLaunch> launch;
    std::vector<int32_t> weak, inc_rows(K), solves(K), leaves(K), cover(K), reopened(K);
    std::vector<double> cost(K), u0((size_t)K * nu), x1((size_t)K * nx), prow((size_t)K * d.n_primal), e0((size_t)K * nx, 0.0);
    size_t used = 0;
    printf("[");
    for (int step = 0; step < steps; step++) {
        for (int k = 0; k < K; k++) tree_begin_step(trees[k], x0s.data() + (size_t)k * nx, nx);
        // (the rows a warm-started tree carries are the first `used` of the pools, as after the library's shift; their
        // contents are the previous step's: reopened leaves are re-solved before anything reads them, which is why -inf
        // bounds make every carried row dead)
        if (fleet_pools_idle(trees)) used = 0;
        pool_dual.resize(used * d.n_dual);
        pool_primal.resize(used * d.n_primal);
        long rounds = 0;
        for (;;) {
            size_t npick = 0;
            for (int k = 0; k < K; k++) { tree_select(trees[k], width, 0.0, picks[k]); npick += picks[k].size(); }
            if (npick == 0) break;
            const size_t B = fleet_count_round(trees, picks, d, ex);
            if (B > 0) {
                std::vector<int8_t> h_fix(B * d.nfix);
                std::vector<int32_t> h_widx(B), status(B), iters(B), polished(B);
                std::vector<double> h_x0(B * nx), obj(B), dobj(B), primal(B * d.n_primal), dual(B * d.n_dual);
                const int any_warm = fleet_fill_round(trees, picks, d, ex, B, h_fix.data(), h_x0.data(), h_widx.data(), launch);
                if (any_warm < 0) { fprintf(stderr, "the two passes over a round disagree\n"); return 4; }
                const int rc = solve(nx, nu, nub, T, nc, ncL, nq, nr, nqT, A.data(), Bm.data(), F.data(), G.data(), h.data(), FT.data(), GT.data(), hT.data(),
                                     Q.data(), R.data(), QT.data(), h_x0.data(), nx, (int)B, h_fix.data(), 1e-8, 1e-6, 100, 4, 1, 1, 1, 1e-4,
                                     any_warm ? pool_primal.data() : nullptr, any_warm ? pool_dual.data() : nullptr, any_warm ? h_widx.data() : nullptr,
                                     obj.data(), dobj.data(), status.data(), iters.data(), primal.data(), dual.data(), polished.data());
                if (rc != 0) { fprintf(stderr, "oracle failed: %d\n", rc); return 3; }
                rounds++;
                for (size_t q = 0; q < B; q++) iters[q] = abi_iters(polished[q]);
                weak.clear();
                fleet_record_round(trees, launch, d, (int32_t)used, B, h_fix.data(), obj.data(), status.data(), iters.data(), dual.data() + d.o_lb, d.n_dual,
                                   ex.dive ? primal.data() : nullptr, d.n_primal, weak);
                for (int32_t q : weak) // (the library writes a dual objective of -inf for these; here every leaf is reopened anyway)
                    if (q < 0 || (size_t)q >= B || status[q] != HMPC_INFEASIBLE) { fprintf(stderr, "weak list: node %d\n", q); return 4; }
                pool_dual.insert(pool_dual.end(), dual.begin(), dual.end());
                pool_primal.insert(pool_primal.end(), primal.begin(), primal.end());
                used += B;
            }
            for (int k = 0; k < K; k++) {
                const int bad = tree_consume(trees[k], picks[k], d.nfix, 0.0);
                if (bad) { fprintf(stderr, "tree_consume: %d\n", bad); return 4; }
            }
        }
        // the incumbents' primal rows, gathered as the library's gather kernel does; then the step's outputs
        if (fleet_incumbent_rows(trees, inc_rows.data()))
            for (int k = 0; k < K; k++)
                if (inc_rows[k] >= 0) std::memcpy(prow.data() + (size_t)k * d.n_primal, pool_primal.data() + (size_t)inc_rows[k] * d.n_primal, d.n_primal * sizeof(double));
        fleet_close_step(trees, d, inc_rows.data(), prow.data(), cost.data(), u0.data(), x1.data(), solves.data(), leaves.data());
        printf("%s[", step ? "," : "");
        for (int k = 0; k < K; k++)
            printf("%s{\"cost\": %.17g, \"solves\": %d, \"leaves\": %d, \"rounds\": %ld}", k ? "," : "", std::isfinite(cost[k]) ? cost[k] : 1e300, solves[k], leaves[k], rounds);
        printf("]");
        // retain / adopt: the next state is the model's (no error); every retained leaf is kept and reopened (bound -inf)
        const size_t Bs = fleet_retain_leaves(trees, d, keep, cover.data(), reopened.data());
        if (Bs > 0) {
            std::vector<double> hx((size_t)K * nx), hu((size_t)K * nu), he((size_t)K * nx), lb(Bs);
            std::vector<int8_t> s_fix(Bs * d.nfix);
            std::vector<int32_t> owner(Bs), src(Bs);
            if (!fleet_stage_shift(trees, d, keep, e0.data(), hx.data(), hu.data(), he.data(), s_fix.data(), owner.data(), src.data(), lb.data())) {
                fprintf(stderr, "a kept leaf carries no multipliers\n");
                return 4;
            }
            lb.assign(Bs, -inf);
            const std::vector<uint8_t> flags(Bs, 3);
            if (!fleet_adopt_shift(trees, d, keep, lb.data(), flags.data(), cover.data(), reopened.data())) return 4;
            used = Bs;
        }
        for (int k = 0; k < K; k++)
            if (trees[k].running) std::memcpy(x0s.data() + (size_t)k * nx, x1.data() + (size_t)k * nx, nx * sizeof(double)); // x_1 of the incumbent
    }
    printf("]\n");
    {   // a node pruned WITHOUT a certificate (HMPC_ITERS_UNCERTIFIED) is counted, with the bound it carried before its solve:
        // what hmpc_fleet_uncertified reports and what decides whether a search's optimum rests on such a prune
        std::vector<FleetTree> one(1);
        FleetTree &t = one[0];
        tree_reset_cold(t, d.nfix);
        tree_begin_step(t, x0s.data(), nx);
        t.lb[0] = 0.25;
        const int32_t status = HMPC_INFEASIBLE, iters = HMPC_ITERS_WEAK | HMPC_ITERS_UNCERTIFIED;
        const std::vector<double> nu_(2 * d.nfix, 0.0);
        const std::vector<FleetLaunch> root{{0, 0}};
        weak.clear();
        fleet_record_round(one, root, d, 0, 1, t.fix.data(), &inf, &status, &iters, nu_.data(), nu_.size(), nullptr, 0, weak);
        const std::vector<int> pk{0};
        if (weak != std::vector<int32_t>{0} || tree_consume(t, pk, d.nfix, 0.0) != 0 || t.uncertified != 1 || t.unc_lb != 0.25 || t.lb[0] != inf ||
            t.solves != 1) {
            fprintf(stderr, "uncertified prune: not accounted for\n");
            return 5;
        }
        tree_begin_step(t, x0s.data(), nx);
        if (t.uncertified != 0 || t.unc_lb != inf) { fprintf(stderr, "uncertified prune: a step does not start clean\n"); return 5; }
    }
    // (no dlclose: the OpenMP runtime the oracle brought in keeps worker threads alive)
    return 0;
}
