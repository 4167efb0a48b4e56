"""Anytime device searches, measured (diagnostic, run by hand; not collected).  Cart-pole with walls, N = 20, 1 / 64 / 1024 trees from
states around X0 (the first is X0 itself, the second the wide tree of tests/test_gpu_search_anytime.py), frontier_width 8, hand-down
off, ONE process.
  A  per rule, a cold search stepped round by round: solves and rounds until a tree's FIRST incumbent and until its optimum is proven
     (median and range over the trees that have one);
  B  rule dive under a budget of m = 8, 16, 32, 64 solves, cold: trees with an incumbent, upper - lower where it is finite, and how
     much of the optimum the proven lower bound has reached (lower / optimum, median and range);
  C  the warm step (advance from a finished best-first step, then run + results + bounds), rule dive under max_solves = m beside the
     unbudgeted best-first step, alternating run by run; each line is the median over the runs with the spread (min .. max) beside
     it -- a difference inside that spread is no difference; and the cost of ONE select on the warm step's covers under every rule
     (the same trees, a search per rule, alternating)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import conftest  # noqa
from time import perf_counter
import numpy as np
np.seterr(invalid='ignore')                                                      # (inf - inf and inf / inf of trees without incumbent: masked out below)
from helpers import make_controller, load_fixture
from warm_start_hmpc_amd.batched import BatchedMPC
from warm_start_hmpc_amd.qp_backend import SEARCH_STATES, SEARCH_STOP_STATES
from warm_start_hmpc_amd.search import DeviceSearch

SIZES = [int(v) for v in os.environ.get('SEARCH_SIZES', '1,64,1024').split(',')]
BUDGETS = [int(v) for v in os.environ.get('SEARCH_BUDGETS', '8,16,32,64').split(',')]
RUNS = int(os.environ.get('SEARCH_RUNS', '5'))
RULES = ('best', 'depth', 'breadth', 'dive')
ctrl = make_controller('cart_pole_with_walls', T=20, backend='hip')
bm = BatchedMPC(ctrl)                                                            # (uploads the shift's maps)
x_max = load_fixture('cart_pole_with_walls')['x_max']
X0 = np.array([0., 0., 1., 0.])
WIDE = np.array([-0.058, 0.016, 0.761, -0.326])
spread = lambda v: '%.4g (%.4g .. %.4g)' % (np.median(v), np.min(v), np.max(v)) if len(v) else 'none'


def states(K):
    rng = np.random.RandomState(7)
    xs = X0 + rng.uniform(-1., 1., (K, 4)) * np.array([.05, .2, .2, .4])
    xs[0] = X0
    if K > 1:
        xs[1] = WIDE
    return xs


def fresh(K, **kw):
    return DeviceSearch(ctrl, K, node_cap=1024, row_cap=8192 + 300 * K, **kw)


for K in SIZES:
    xs = states(K)
    errs = np.array([0.001 * np.random.RandomState(s).randn(4) * x_max for s in range(K)])
    # ---- A: solves and rounds to the first incumbent and to the optimum, per rule
    opt = None
    for rule in RULES:
        ds = fresh(K, rule=rule)
        ds.begin(xs)
        first_s, first_r = np.full(K, -1), np.full(K, -1)
        rounds = 0
        while ds.run(8, 0., False, max_rounds=1)[0]:
            rounds += 1
            r = ds.results()
            new = np.isfinite(r['cost']) & (first_s < 0)
            first_s[new], first_r[new] = r['solves'][new], rounds
        r = ds.results()
        assert not (r['state'] & (SEARCH_STATES['failed'] | SEARCH_STATES['overflow'])).any()
        fin = np.isfinite(r['cost'])
        if opt is None:
            opt = r['cost'].copy()
        assert np.array_equal(fin, np.isfinite(opt)) and np.allclose(r['cost'][fin], opt[fin], rtol=1e-5, atol=0.)
        print('A %4d trees (%d feasible), %-7s: first incumbent after %s solves, %s rounds; optimum proven after %s solves, %d rounds'
              % (K, fin.sum(), rule, spread(first_s[fin]), spread(first_r[fin]), spread(r['solves'][fin]), rounds), flush=True)
        del ds
    # ---- B: what a cold dive has proved after m solves
    fin = np.isfinite(opt)
    ds = fresh(K, rule='dive')
    for m in BUDGETS:
        ds.set_budget(m)
        ds.begin(xs)
        ds.run(8, 0., False)
        r, b = ds.results(), ds.bounds()
        has = (r['state'] & SEARCH_STATES['incumbent']) != 0
        cut = (r['state'] & SEARCH_STOP_STATES['budget']) != 0
        print('B %4d trees, dive, m = %3d: %d cut off, %d of them with an incumbent; upper - lower %s; lower / optimum %s'
              % (K, m, cut.sum(), (cut & has).sum(), spread((b['upper'] - b['lower'])[has]), spread((b['lower'] / opt)[fin])), flush=True)
    del ds
    # ---- C: the warm step, dive under a budget beside unbudgeted best-first
    def warm_step(ds, rule, m):
        ds.set_rule('best')
        ds.set_budget(None)
        ds.begin(xs)
        ds.run(8, 0., False)
        ds.results()
        ds.set_rule(rule)
        ds.set_budget(m)
        tic = perf_counter()
        ds.advance(errs, stats=False)
        ds.run(8, 0., False)
        r, b = ds.results(), ds.bounds()
        toc = perf_counter()
        return toc - tic, r, b

    ds = fresh(K)
    warm_step(ds, 'best', None)                                                 # warm-up: allocations, kernels' first-use checks
    plans = [('best', None)] + [('dive', m) for m in BUDGETS] + [('dive', None)]
    times = {p: [] for p in plans}
    last = {}
    for i in range(RUNS):
        for p in plans:                                                         # alternating: every plan once per pass
            t, r, b = warm_step(ds, *p)
            times[p].append(1e3 * t)
            last[p] = (r, b)
    base = last[('best', None)][0]['cost']
    for p in plans:
        r, b = last[p]
        cut = (r['state'] & SEARCH_STOP_STATES['budget']) != 0
        has = np.isfinite(r['cost'])
        worse = (r['cost'][has] - base[has]) / base[has]
        print('C %4d trees, %-4s m = %-4s: warm step %s ms; solves %s; %d cut off (%d without incumbent); cost above the optimum %s; upper - lower %s'
              % (K, p[0], p[1], spread(times[p]), spread(r['solves']), cut.sum(), (cut & ~has).sum(), spread(worse), spread((b['upper'] - b['lower'])[has])), flush=True)
    del ds
    # one select on the warm step's covers, per rule
    per = {}
    for rule in RULES:
        s = fresh(K)
        s.begin(xs)
        s.run(8, 0., False)
        s.advance(errs, stats=False)
        s.set_rule(rule)
        s.select(8, 0., False)                                                  # (warm-up; a select that is not consumed is staged again)
        per[rule] = (s, [])
    for i in range(4 * RUNS):
        for rule in RULES:
            s, t = per[rule]
            tic = perf_counter()
            s.select(8, 0., False)
            t.append(1e6 * (perf_counter() - tic))
    print('C %4d trees, one select (four kernels, one readback): %s' % (K, ';  '.join('%s %s us' % (rule, spread(per[rule][1])) for rule in RULES)), flush=True)
    del per
