"""A cold and a warm MPC step of 1 / 64 / 1024 device-resident searches at speculation depths 0, 1 and 2, beside FleetMPC.solve at
the same depth, in ONE process (diagnostic, run by hand; not collected).  Cart-pole with walls, N = 20, sigma = 0.001,
frontier_width 8, hand-down off (so that every depth is the same search).  Per size and depth: one warm-up pass, then RUNS runs
alternating between the two paths; each line is the median over the runs with the spread (min .. max) beside it -- a difference
inside that spread is no difference.  'cold step': begin + run + results (fleet: reset + solve); 'warm step': advance + run +
results (fleet: shift + solve), what a closed loop pays per step.  Both ends synchronise.  The costs of the two paths are asserted
equal at every step; launches / rows are those of the warm step (the search's counters; the fleet's stats)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import conftest  # noqa
from time import perf_counter
import numpy as np
from helpers import make_controller, load_fixture
from warm_start_hmpc_amd.batched import BatchedMPC
from warm_start_hmpc_amd.fleet import FleetMPC
from warm_start_hmpc_amd.search import DeviceSearch

SIZES = [int(v) for v in os.environ.get('SEARCH_SIZES', '1,64,1024').split(',')]
DEPTHS = [int(v) for v in os.environ.get('SEARCH_DEPTHS', '0,1,2').split(',')]
RUNS = int(os.environ.get('SEARCH_RUNS', '5'))
ctrl = make_controller('cart_pole_with_walls', T=20, backend='hip')
bm = BatchedMPC(ctrl)                                                            # (uploads the shift's maps)
x_max = load_fixture('cart_pole_with_walls')['x_max']
X0 = np.array([0., 0., 1., 0.])


def search_steps(ds, xs, errs):
    tic = perf_counter()
    ds.begin(xs)
    ds.run(8, 0., False)
    r1 = ds.results()
    mid = perf_counter()
    ds.advance(errs)
    before = ds.counters()
    ds.run(8, 0., False)
    r2 = ds.results()
    toc = perf_counter()
    after = ds.counters()
    return mid - tic, toc - mid, r1['cost'], r2['cost'], after['launches'] - before['launches'], after['rows'] - before['rows']


def fleet_steps(fl, xs, errs, depth):
    fl.reset()
    tic = perf_counter()
    r1 = fl.solve(xs, 8, speculation=depth)
    mid = perf_counter()
    before = fl.stats()
    tic2 = perf_counter()
    fl.shift(errs)
    r2 = fl.solve(r1['x1'] + errs, 8, speculation=depth)
    toc = perf_counter()
    after = fl.stats()
    return mid - tic, toc - tic2, r1['cost'], r2['cost'], after['rounds'] - before['rounds'], after['launched'] - before['launched']


for K in SIZES:
    xs = np.repeat(X0[None], K, axis=0)
    errs = np.array([0.001 * np.random.RandomState(s).randn(4) * x_max for s in range(K)])
    for depth in DEPTHS:
        ds = DeviceSearch(ctrl, K, node_cap=1024, row_cap=max(4096, 300 * K * (2 ** (depth + 1) - 1)), speculation=depth)
        fl = FleetMPC(ctrl, K, handdown=False)
        search_steps(ds, xs, errs), fleet_steps(fl, xs, errs, depth)             # warm-up: allocations, kernels' first-use checks
        t = {'search': [], 'fleet': []}
        for i in range(RUNS):
            a, b = search_steps(ds, xs, errs), fleet_steps(fl, xs, errs, depth)
            assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), (K, depth, a[2:4], b[2:4])
            t['search'].append(a)
            t['fleet'].append(b)
        for name in ('search', 'fleet'):
            v = 1e3 * np.array([r[:2] for r in t[name]])
            print('%4d trees, depth %d, %-6s: cold step %8.2f ms (%.2f .. %.2f)   warm step %8.2f ms (%.2f .. %.2f)   [%d launches, %d rows]'
                  % (K, depth, name, np.median(v[:, 0]), v[:, 0].min(), v[:, 0].max(), np.median(v[:, 1]), v[:, 1].min(), v[:, 1].max(),
                     t[name][-1][4], t[name][-1][5]), flush=True)
        del ds, fl
