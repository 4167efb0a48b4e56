"""What a controller waits for between a measurement and an input, with and without the search moved into the idle time: ten closed-loop
steps of 1 / 64 / 1024 device-resident searches as DeviceSearch.closed_loop(resident=True) walks them (advance with the measured
error -> run -> results) and as closed_loop(presolve=True) does (advance to the predicted state -> run in the idle time | re-base to the
measurement -> run -> results), in ONE process (diagnostic, run by hand; not collected).  Cart-pole with walls, N = 20, the published
errors of sigma = 0.001 / 0.003 / 0.010 (tests/golden/reference_closed_loop.npz, cycled beyond their 100 trajectories), frontier_width
8, hand-down on.  Per noise level and size: one warm-up pass, then RUNS runs alternating between the two; every line is the median
over runs and steps 1 .. 9 with the spread (min .. max) beside it -- a difference inside that spread is no difference.
  resident  warm step: advance + run + results, its rounds and its solves per tree
  presolve  run time: re-base + run + results, its rounds (rounds_rt), solves per tree (nodes_rt) and reopened leaves per tree
            (reopened_rt); idle time: advance + run + results at the predicted state, its solves per tree (nodes_pre)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import conftest  # noqa
from time import perf_counter
import numpy as np
from helpers import make_controller, load_fixture
from warm_start_hmpc_amd.search import DeviceSearch

SIZES = [int(v) for v in os.environ.get('SEARCH_SIZES', '1,64,1024').split(',')]
NOISE = os.environ.get('SEARCH_NOISE', '0001,0003,0010').split(',')
RUNS = int(os.environ.get('SEARCH_RUNS', '5'))
STEPS = 10
ctrl = make_controller('cart_pole_with_walls', T=20, backend='hip')
published = load_fixture('reference_closed_loop')
X0 = np.array([0., 0., 1., 0.])


class Timed(DeviceSearch):
    """Every run / advance / results of a closed loop with its wall time (all three synchronise) and, for a run, its rounds."""

    def _timed(self, name, call, *a, **kw):
        tic = perf_counter()
        out = call(*a, **kw)
        self.log.append((name, perf_counter() - tic, out[0] if name == 'run' else 0))
        return out

    def run(self, *a, **kw):
        return self._timed('run', super().run, *a, **kw)

    def advance(self, *a, **kw):
        return self._timed('advance', super().advance, *a, **kw)

    def results(self, *a, **kw):
        return self._timed('results', super().results, *a, **kw)


def resident(ds, errors):
    """Per warm step (1 .. STEPS - 1): seconds of advance + run + results, rounds; and the solves per tree."""
    ds.log = []
    out = ds.closed_loop(X0, STEPS, errors, resident=True)
    n = len(ds.log) // 3                                                         # (fewer than STEPS where every loop has ended: the walk stops there)
    names = [e[0] for e in ds.log[:3 * n]]
    assert names == ['run', 'results', 'advance'] * n, names
    t = np.array([e[1] for e in ds.log[:3 * n]]).reshape(n, 3)
    rounds = np.array([e[2] for e in ds.log[:3 * n]]).reshape(n, 3)[:, 0]
    return t[:-1, 2] + t[1:, 0] + t[1:, 1], rounds[1:], out['nodes_ws'][:, 1:], out['costs']


def line(name, v, fmt='%8.2f'):
    v = np.asarray(v, dtype=np.float64).ravel()
    return ('%s ' + fmt + ' (' + fmt.strip() + ' .. ' + fmt.strip() + ')') % (name, np.median(v), v.min(), v.max())


for noise in NOISE:
    for K in SIZES:
        errors = published['errors_' + noise][np.arange(K) % 100, :STEPS]
        rs, ps = (Timed(ctrl, K, node_cap=1024, row_cap=max(8192, 600 * K)) for _ in range(2))
        ps.log = []
        resident(rs, errors), ps.closed_loop(X0, STEPS, errors, presolve=True)      # warm-up: allocations, kernels' first-use checks
        acc = dict(res_t=[], res_rounds=[], res_nodes=[], rt_t=[], rt_rounds=[], rt_nodes=[], reopened=[], pre_t=[], pre_nodes=[])
        for i in range(RUNS):
            t, rounds, nodes, costs = resident(rs, errors)
            ps.log = []
            p = ps.closed_loop(X0, STEPS, errors, presolve=True)
            ended = np.isnan(costs)
            assert np.array_equal(ended, np.isnan(p['costs'])) and np.all(np.isclose(costs, p['costs'], rtol=1e-5) | ended)
            live = ~ended[:, 1:]
            acc['res_t'].append(1e3 * t), acc['res_rounds'].append(rounds), acc['res_nodes'].append(nodes[live])
            ran = p['time_rt'][1:] > 0.                                           # (the steps the walk reached)
            acc['rt_t'].append(1e3 * p['time_rt'][1:][ran]), acc['rt_rounds'].append(p['rounds_rt'][1:][ran]), acc['rt_nodes'].append(p['nodes_rt'][:, 1:][live])
            acc['reopened'].append(p['reopened_rt'][:, 1:][live]), acc['pre_t'].append(1e3 * p['time_pre'][1:][ran]), acc['pre_nodes'].append(p['nodes_pre'][:, 1:][live])
        cat = {k: np.concatenate([np.ravel(a) for a in v]) for k, v in acc.items()}
        print('sigma 0.%s, %4d trees, resident: %s   %s   %s' % (noise[1:], K, line('warm step ms', cat['res_t']), line('rounds', cat['res_rounds'], '%5.1f'),
                                                                line('solves / tree', cat['res_nodes'], '%6.1f')), flush=True)
        print('sigma 0.%s, %4d trees, presolve: %s   %s   %s   %s' % (noise[1:], K, line('run time  ms', cat['rt_t']), line('rounds', cat['rt_rounds'], '%5.1f'),
                                                                     line('solves / tree', cat['rt_nodes'], '%6.1f'), line('reopened / tree', cat['reopened'], '%6.1f')), flush=True)
        print('sigma 0.%s, %4d trees, presolve: %s   %s' % (noise[1:], K, line('idle time ms', cat['pre_t']), line('solves / tree', cat['pre_nodes'], '%6.1f')), flush=True)
        del rs, ps
