"""The step boundary of 1 / 64 / 1024 device-resident searches, on the host path (leaves down, hmpc_shift_batch through host arrays,
begin up: the code DeviceSearch.closed_loop runs by default) and on the device (DeviceSearch.advance), in ONE process (diagnostic,
run by hand; not collected).  Cart-pole with walls, N = 20, sigma = 0.001, frontier_width 8, hand-down on.  Per size: RUNS runs
alternating between the two, each a cold step, the boundary and a warm step on a search of its own; the line of each is the median
over the runs with the spread (min .. max) beside it -- a difference inside that spread is no difference.  'boundary': from the
results of the cold step to a search that is ready to select; 'warm step': boundary + run + results, what a closed loop pays per
step.  Both ends synchronise (results before, a select's readback after), so the wall clock sees the device work."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import conftest  # noqa
from time import perf_counter
import numpy as np
from helpers import make_controller, load_fixture
from warm_start_hmpc_amd.batched import BatchedMPC
from warm_start_hmpc_amd.search import DeviceSearch

SIZES = [int(v) for v in os.environ.get('SEARCH_SIZES', '1,64,1024').split(',')]
RUNS = int(os.environ.get('SEARCH_RUNS', '5'))
ctrl = make_controller('cart_pole_with_walls', T=20, backend='hip')
bm = BatchedMPC(ctrl)
x_max = load_fixture('cart_pole_with_walls')['x_max']
X0 = np.array([0., 0., 1., 0.])


def cold(ds, K):
    xs = np.repeat(X0[None], K, axis=0)
    ds.begin(xs)
    ds.run(8)
    return xs, ds.results()


def warm(ds, tic, mid):
    ds.run(8)
    r2 = ds.results()
    toc = perf_counter()
    return mid - tic, toc - tic, r2['cost']


def host_steps(ds, K, errs):
    xs, r = cold(ds, K)
    tic = perf_counter()
    ws = bm.construct_warm_start_many(ds.leaves(), xs, r['u0'], errs)
    ds.begin(r['x1'] + errs, ws)
    return warm(ds, tic, perf_counter())


def device_steps(ds, K, errs):
    xs, r = cold(ds, K)
    tic = perf_counter()
    ds.advance(errs)                                                             # (with cover / reopened, as closed_loop asks: it waits for the adopt kernel)
    return warm(ds, tic, perf_counter())


for K in SIZES:
    errs = np.array([0.001 * np.random.RandomState(s).randn(4) * x_max for s in range(K)])
    hs, rs = (DeviceSearch(ctrl, K, node_cap=1024, row_cap=max(4096, 600 * K)) for _ in range(2))
    host_steps(hs, K, errs), device_steps(rs, K, errs)                           # warm-up: allocations, kernels' first-use checks
    t = {'host': [], 'advance': []}
    for i in range(RUNS):
        a, b = host_steps(hs, K, errs), device_steps(rs, K, errs)
        assert np.array_equal(a[2], b[2], equal_nan=True)
        t['host'].append(a[:2])
        t['advance'].append(b[:2])
    for name in ('host', 'advance'):
        v = 1e3 * np.array(t[name])
        print('%4d trees, %-7s: boundary %8.2f ms (%.2f .. %.2f)   warm step %8.2f ms (%.2f .. %.2f)'
              % (K, name, np.median(v[:, 0]), v[:, 0].min(), v[:, 0].max(), np.median(v[:, 1]), v[:, 1].min(), v[:, 1].max()), flush=True)
    del hs, rs
