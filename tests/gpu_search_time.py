"""A cold and a warm MPC step of 1 / 64 / 1024 searches through DeviceSearch.run (trees, selection and consumption on the device)
and through FleetMPC.solve (trees on the host, the path the fleet takes), in ONE process (diagnostic, run by hand; not collected).
Cart-pole with walls, N = 20, sigma = 0.001, frontier_width 8, hand-down on for both.  Per size: RUNS runs alternating between the
two, each a cold step, a shift and a warm step; the line of each is the median over the runs with the spread (min .. max) beside
it -- a difference inside that spread is no difference.  The device search's step includes its begin (covers up) and, for the
warm step, the leaves (down) and the shift through the host arrays; the fleet shifts in place: the 'solve' columns compare the
searches alone."""
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
RUNS = int(os.environ.get('SEARCH_RUNS', '5'))
ctrl = make_controller('cart_pole_with_walls', T=20, backend='hip')
bm = BatchedMPC(ctrl)
x_max = load_fixture('cart_pole_with_walls')['x_max']
X0 = np.array([0., 0., 1., 0.])


def device_steps(ds, K, errs):
    xs = np.repeat(X0[None], K, axis=0)
    tic = perf_counter()
    ds.begin(xs)
    ds.run(8)
    r = ds.results()
    cold = perf_counter() - tic
    leaves = ds.leaves()
    ws = bm.construct_warm_start_many(leaves, xs, r['u0'], errs)
    xs = r['x1'] + errs
    tic = perf_counter()
    ds.begin(xs, ws)
    mid = perf_counter()
    ds.run(8)
    r2 = ds.results()
    return cold, perf_counter() - tic, perf_counter() - mid, r['cost'], r2['cost']


def fleet_steps(fl, K, errs):
    fl.reset()
    xs = np.repeat(X0[None], K, axis=0)
    tic = perf_counter()
    r = fl.solve(xs, 8)
    cold = perf_counter() - tic
    fl.shift(errs)
    tic = perf_counter()
    r2 = fl.solve(r['x1'] + errs, 8)
    warm = perf_counter() - tic
    return cold, warm, warm, r['cost'], r2['cost']


for K in SIZES:
    errs = np.array([0.001 * np.random.RandomState(s).randn(4) * x_max for s in range(K)])
    ds, fl = DeviceSearch(ctrl, K, node_cap=1024, row_cap=max(4096, 600 * K)), FleetMPC(ctrl, K)
    device_steps(ds, K, errs), fleet_steps(fl, K, errs)                          # warm-up: allocations, kernels' first-use checks
    t = {'device': [], 'fleet': []}
    for i in range(RUNS):
        a, b = device_steps(ds, K, errs), fleet_steps(fl, K, errs)
        np.testing.assert_allclose(a[3], b[3], rtol=1e-9)
        np.testing.assert_allclose(a[4], b[4], rtol=1e-9)
        t['device'].append(a[:3])
        t['fleet'].append(b[:3])
    for name in ('device', 'fleet'):
        v = 1e3 * np.array(t[name])
        print('%4d trees, %-6s: cold step %8.2f ms (%.2f .. %.2f)   warm step %8.2f ms (%.2f .. %.2f)   warm solve alone %8.2f ms (%.2f .. %.2f)'
              % (K, name, np.median(v[:, 0]), v[:, 0].min(), v[:, 0].max(), np.median(v[:, 1]), v[:, 1].min(), v[:, 1].max(),
                 np.median(v[:, 2]), v[:, 2].min(), v[:, 2].max()), flush=True)
    del ds, fl
