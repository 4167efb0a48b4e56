"""Warm steps of the 1024-loop fleet of bench.py (cart-pole with walls, N = 20, sigma = 0.001, frontier_width 8, no speculation,
hand-down on) with the digest of a round off (the default path) and on, in ONE process (diagnostic, run by hand; not collected).
Per run: a cold step and STEPS warm steps; per warm step the five slots of hmpc_fleet_timing; MPC steps/s over the warm steps with
the first one dropped.  The two settings alternate run by run; the line of each is the median over RUNS runs, with the spread
(min .. max) beside it -- a difference inside that spread is no difference."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import conftest  # noqa
from time import perf_counter
import numpy as np
from helpers import make_controller, load_fixture
from warm_start_hmpc_amd.fleet import FleetMPC

K = int(os.environ.get('DIGEST_LOOPS', '1024'))
STEPS = int(os.environ.get('DIGEST_STEPS', '10'))
RUNS = int(os.environ.get('DIGEST_RUNS', '5'))
SPEC = int(os.environ.get('DIGEST_SPECULATION', '0'))
SLOTS = ('select', 'stage', 'device', 'consume', 'shift')
ctrl = make_controller('cart_pole_with_walls', T=20, backend='hip')
x_max = load_fixture('cart_pole_with_walls')['x_max']
errs = np.array([0.001 * np.random.RandomState(s).randn(STEPS + 1, 4) * x_max for s in range(K)])
X0 = np.array([0., 0., 1., 0.])
fleets = {False: FleetMPC(ctrl, K, digest=False), True: FleetMPC(ctrl, K, digest=True)}


def run(fl, show):
    """One closed loop of STEPS + 1 steps; (steps/s over warm steps 2 .. STEPS, per-slot ms per warm step, costs)."""
    fl.reset()
    xs = np.repeat(X0[None], K, axis=0)
    walls, slots, costs = [], [], []
    for t in range(STEPS + 1):
        before = fl.stats()['seconds']
        tic = perf_counter()
        r = fl.solve(xs, 8, speculation=SPEC)
        fl.shift(errs[:, t])
        walls.append(perf_counter() - tic)
        after = fl.stats()['seconds']
        slots.append([1e3 * (after[k] - before[k]) for k in SLOTS])
        costs.append(r['cost'].copy())
        if show and t > 0:
            print('    step %2d: %7.3f ms   ' % (t, 1e3 * walls[-1]) + '  '.join('%s %6.3f' % (k, v) for k, v in zip(SLOTS, slots[-1])), flush=True)
        xs = r['x1'] + errs[:, t]
    warm = walls[2:]                                                             # (the cold step and the first warm step dropped)
    return K * len(warm) / sum(warm), np.mean(slots[2:], axis=0), np.array(costs)


for digest in (False, True):                                                     # warm-up: allocations, kernels' first-use checks
    run(fleets[digest], False)
rates, parts, costs = {False: [], True: []}, {False: [], True: []}, {}
for i in range(RUNS):
    for digest in (False, True):
        print('run %d, digest %s' % (i, 'on' if digest else 'off'), flush=True)
        rate, slot, cost = run(fleets[digest], i == 0)
        rates[digest].append(rate)
        parts[digest].append(slot)
        costs[digest] = cost
assert np.array_equal(costs[False], costs[True]), 'the digest changed a cost'
for digest in (False, True):
    v, s = np.array(rates[digest]), np.median(np.array(parts[digest]), axis=0)
    print('digest %-3s: %d loops, %d warm steps x %d runs: median %.0f MPC steps/s (min %.0f, max %.0f); ms per warm step: %s'
          % ('on' if digest else 'off', K, STEPS - 1, RUNS, np.median(v), v.min(), v.max(), '  '.join('%s %.3f' % (k, x) for k, x in zip(SLOTS, s))), flush=True)
