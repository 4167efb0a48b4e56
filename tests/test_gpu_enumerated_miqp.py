"""The HIP backend held to the exhaustively enumerated optimum (tests/enumeration_reference.py; the truth comes from the CPU oracle,
once per problem and state):

  * the kernels enumerate: all leaves of a workload in one ``solve_batch`` -- every node fully fixed in every stage, the narrow stage
    body and the narrow panel throughout -- on the shipped run-time-sized kernel at 1 / 2 / 4 waves, its streaming form and the
    compiled kernels: statuses exactly, objectives as ``test_gpu_parity._compare`` holds them;
  * every search path -- ``controller.feedforward``, ``BatchedMPC.feedforward_many``, ``FleetMPC.solve``, ``DeviceSearch`` under every
    rule, with and without speculation and hand-down, at width 1 and 8 -- finds the enumerated optimum with its binaries, u0 and
    x1, and leaves a partition of the cube whose every bound is one;
  * step boundaries -- the fleet's shift, the host shift under both shift kernels, ``advance``, ``rebase`` -- carry covers whose
    every bound is a lower bound of its part of the NEXT state's problem;
  * an anytime search brackets the optimum at every stop.

The cart-pole workloads (T = 3) and the streaming form run the shipped kernels: nothing here compiles on the GPU machine (the
compiled kernels of the random MLDs are those of tests/jit_problems.py)."""
import contextlib
import os

import numpy as np
import pytest

import anytime_reference as ar
import branch_reference as br
import enumeration_reference as en
import search_reference as sr
from certificates import EXTRA_LINES
from warm_start_hmpc_amd import branch_and_bound as bb

pytestmark = pytest.mark.gpu
FAMILIES = {'default': ({}, {}), 'shipped_w1': (dict(HMPC_JIT=0), dict(HMPC_WAVES=1)), 'shipped_w2': (dict(HMPC_JIT=0), dict(HMPC_WAVES=2)),
            'shipped_w4': (dict(HMPC_JIT=0), dict(HMPC_WAVES=4)), 'streaming': (dict(HMPC_FORCE_BIG=1), {})}    # (at creation, at launch)
KINDS = {'default': 6, 'shipped_w1': 0, 'shipped_w2': 0, 'shipped_w4': 0, 'streaming': 1}                        # hmpc_kernel_info of the random MLDs
RULES = {'best': bb.best_first, 'depth': bb.depth_first, 'breadth': bb.breadth_first}
STEPS = 3
_HANDLES, _ORACLES = {}, {}
WORST = {}                 # path -> worst (lb - below) / (1 + |below|) of this session, written out at its end


@contextlib.contextmanager
def _env(**values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update({k: str(v) for k, v in values.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _oracle(name):
    if name not in _ORACLES:
        _ORACLES[name] = en.controller(name, threads=8)
    return _ORACLES[name]


def _truth(name, x0):
    return en.truth(_oracle(name), x0)


def _backend(name, family='default'):
    """(controller on a HipBatchedQP, dims), one handle per problem and family, kept -- the manner of tests/test_gpu_branch.py::_backend."""
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    if (name, family) not in _HANDLES:
        ctrl = en.controller(name, backend=None)
        with _env(**FAMILIES[family][0]):
            ctrl.qp = HipBatchedQP(ctrl.problem_data())
        d = br.dims_of(ctrl.problem_data())
        assert (d['n_primal'], d['n_dual']) == (ctrl.qp.n_primal, ctrl.qp.n_dual)
        _HANDLES[name, family] = (ctrl, d)
    return _HANDLES[name, family]


def _search_backend(name):
    """The family the searches run on: the compiled kernels of the random MLDs, the shipped ones of the cart-pole at T = 3."""
    return _backend(name, 'shipped_w1' if name in en.CART_POLES else 'default')


def _note(path, report):
    print(path, report.figures())
    if report.kind == 'bounds' and report.finite:
        WORST[path] = max(WORST.get(path, -np.inf), report.worst)


@pytest.fixture(scope='module', autouse=True)
def _report_worst_overshoots():
    yield
    line = 'enumerated MIQP, worst (lb - below) / (1 + |below|) per path of this run: ' + '; '.join('%s %.3g' % kv for kv in sorted(WORST.items()))
    print('\n' + line)
    EXTRA_LINES.append(line)                                # (written out beside the parity margins by tests/test_gpu_parity.py, which runs later in a session)


def _errors(nx, sd, K):
    return sd * np.random.default_rng(7).standard_normal((K, STEPS, nx))


def _loop_states(name):
    return en.states(name)[:3]                                                 # x0 * (0.3, 1, 2): every loop keeps a solution for three steps on the oracle


# ---- the kernels enumerate -----------------------------------------------------------------------------------------------------------
CASES = ([(n, f) for n in en.SMALL for f in FAMILIES] + [('random_mld_t5', 'default'), ('random_mld_t5', 'shipped_w4')] +
         [(n, 'shipped_w%d' % w) for n in en.CART_POLES for w in (1, 2, 4)])


@pytest.mark.parametrize('name,family', CASES)
def test_all_leaves_in_one_launch_are_the_oracles_leaves(name, family):
    ctrl, d = _backend(name, family)
    qp = ctrl.qp
    if name not in en.CART_POLES:
        assert qp.kernel_info() == (KINDS[family],) * 3, qp.kernel_info()
    leaves = en.all_leaves(d['nfix'])
    worst = 0.
    for s, x0 in enumerate(en.states(name)):
        b = _truth(name, x0).rec
        with _env(**FAMILIES[family][1]):
            a = qp.solve_batch(x0, leaves)
        what = (name, family, s)
        assert np.array_equal(a['status'], b['status']), (what, np.flatnonzero(a['status'] != b['status'])[:8])
        fin, inf = a['status'] == 0, a['status'] == 1
        if fin.any():
            worst = max(worst, float(np.max(np.abs(a['obj'][fin] - b['obj'][fin]) / (1. + np.abs(b['obj'][fin])))))
        print(what, '%d optimal, %d infeasible, objectives within %.3g' % (fin.sum(), inf.sum(), worst))
        # the objective lines of tests/test_gpu_parity.py::_compare (polished or not: the same two tolerances there)
        np.testing.assert_allclose(a['obj'][fin], b['obj'][fin], rtol=1e-8, atol=1e-11, err_msg=str(what))
        np.testing.assert_allclose(a['dual_obj'][fin], b['dual_obj'][fin], rtol=1e-6, atol=1e-9, err_msg=str(what))
        assert np.all(np.isinf(a['obj'][inf])) and np.all(np.isnan(a['primal'][inf])), what
        t = _truth(name, x0)
        if t.feasible:                                                          # the row the plant would be driven by
            k = int(np.argmin(np.where(fin, a['obj'], np.inf)))
            n = (t.T + 1) * t.nx
            en.hold(en.result(t, a['obj'][k], leaves[k], a['primal'][k][n:n + t.nu], a['primal'][k][t.nx:2 * t.nx]), what)
    if family == 'default':
        assert qp.jit_stats()[0] == 0, qp.jit_stats()                           # no compiled kernel was dropped


# ---- every search path ---------------------------------------------------------------------------------------------------------------
def _hold_many(name, x0s, out, what, tol=0.):
    """The list of dicts of feedforward_many (either driver) against the truths: result, bounds, cover.  Returns the merged bounds report."""
    worst = en.Report('bounds')
    for k, r in enumerate(out):
        t = _truth(name, x0s[k])
        if r['ub'] is None:
            en.hold(en.result(t, r['objective'], None), (what, k))
        else:
            en.hold(en.result(t, r['objective'], r['ub'], np.concatenate((r['uc'][0], r['ub'][0])), r['x'][1], tol=tol), (what, k))
        worst.merge(en.hold_tree(t, r['leaves'].fix, r['leaves'].lb, (what, k)))
    return worst


@pytest.mark.parametrize('rule', list(RULES))
@pytest.mark.parametrize('name', en.SMALL + tuple(en.CART_POLES))
def test_feedforward_on_the_device_finds_the_enumerated_optimum(name, rule):
    ctrl, d = _search_backend(name)
    xs = en.states(name)
    worst = en.Report('bounds')
    for kw in ({}, dict(handdown=True, speculation_depth=2, frontier_width=8, tol=0.05)):
        for s, x0 in enumerate(xs if len(xs) < 5 else xs[[1, 4]]):
            t = _truth(name, x0)
            sol, leaves, solves, _ = ctrl.feedforward(x0, search_rule=RULES[rule], printing_period=None, **kw)
            what = (name, rule, sorted(kw), s)
            if sol is None:
                en.hold(en.result(t, np.inf, None), what)
            else:
                v = sol.variables
                en.hold(en.result(t, sol.objective, v['ub'], np.concatenate((v['uc'][0], v['ub'][0])), v['x'][1], tol=kw.get('tol', 0.)), what)
            fix = np.array([ctrl._fix_vector(l.identifier) for l in leaves], np.int8).reshape(len(leaves), d['nfix'])
            worst.merge(en.hold_tree(t, fix, [l.lb for l in leaves], what))
    _note('feedforward', worst)


@pytest.mark.parametrize('name', en.SMALL + tuple(en.CART_POLES))
def test_the_numpy_driver_on_the_device_finds_the_enumerated_optima(name):
    from warm_start_hmpc_amd.batched import BatchedMPC
    ctrl, d = _search_backend(name)
    x0s = en.states(name)
    _note('BatchedMPC', _hold_many(name, x0s, BatchedMPC(ctrl).feedforward_many(x0s, None, frontier_width=8), (name, 'batched')))


@pytest.mark.parametrize('handdown,digest', [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize('name', en.SMALL)
def test_the_fleet_finds_the_enumerated_optima_with_their_inputs(name, handdown, digest):
    from warm_start_hmpc_amd.fleet import FleetMPC
    ctrl, d = _search_backend(name)
    x0s = en.states(name)
    fl = FleetMPC(ctrl, len(x0s), handdown=handdown, digest=digest)
    for spec in (0, 2, -1):
        fl.reset()
        r = fl.solve(x0s, frontier_width=8, speculation=spec)
        for k in range(len(x0s)):
            t = _truth(name, x0s[k])
            # (the fleet returns no binaries: u0 and x1 are held to the argmin leaf's row; what u0 holds without a solution is not documented)
            got = en.hold(en.result(t, r['cost'][k], None, r['u0'][k] if t.feasible else None, r['x1'][k] if t.feasible else None), (name, handdown, digest, spec, k))
        print(name, handdown, digest, spec, 'costs', r['cost'], 'solves', r['solves'], got.figures())


@pytest.mark.parametrize('rule', ['best', 'depth', 'breadth', 'dive'])
@pytest.mark.parametrize('name', en.SMALL)
def test_device_searches_find_the_enumerated_optima_under_every_rule(name, rule):
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, d = _search_backend(name)
    x0s = en.states(name)
    K, cap = len(x0s), 8192                                                     # (a tree of 2^12 leaves has 8191 nodes)
    worst = en.Report('bounds')
    for spec in (0, 2):
        ds = DeviceSearch(ctrl, K, node_cap=cap, row_cap=K * cap * (4 if spec else 1), speculation=spec, rule=rule)
        for handdown in (True, False):
            for width in (1, 8):
                out = ds.feedforward_many(x0s, None, frontier_width=width, tol=0., handdown=handdown)
                worst.merge(_hold_many(name, x0s, out, (name, rule, spec, handdown, width)))
                res = ds.results()
                for k in range(K):                                              # `run` / `results`: the same answer in the search's own words
                    t = _truth(name, x0s[k])
                    en.hold(en.result(t, res['cost'][k], res['binaries'][k] if t.feasible else None, res['u0'][k], res['x1'][k]), (name, rule, spec, handdown, width, k))
                assert np.all(res['state'] & sr.DONE)
        del ds
    _note('DeviceSearch %s' % rule, worst)


# ---- step boundaries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sd', [0., 0.05])
@pytest.mark.parametrize('name', en.SMALL)
def test_the_fleets_loop_applies_the_enumerated_inputs_and_keeps_the_oracles_covers(name, sd):
    from warm_start_hmpc_amd.batched import BatchedMPC
    from warm_start_hmpc_amd.fleet import FleetMPC
    ctrl, d = _search_backend(name)
    orc = _oracle(name)
    bm = BatchedMPC(orc)
    xs = _loop_states(name)
    K = len(xs)
    e = _errors(d['nx'], sd, K)
    fl = FleetMPC(ctrl, K)
    fl.reset()
    ws = [None] * K
    for step in range(STEPS):
        r = fl.solve(xs, frontier_width=8)
        ref = bm.feedforward_many(xs, ws, frontier_width=8)
        for k in range(K):
            t = _truth(name, xs[k])
            assert t.feasible, (name, sd, step, k)
            en.hold(en.result(t, r['cost'][k], None, r['u0'][k], r['x1'][k]), (name, sd, step, k))
        cover, reopened = fl.shift(e[:, step])
        ws = [bm.construct_warm_start(ref[k]['leaves'], xs[k], ref[k]['uc'][0], ref[k]['ub'][0], e[k, step]) for k in range(K)]
        print(name, sd, step, 'cover', cover, 'oracle', [len(w) for w in ws], 'reopened', reopened)
        assert np.array_equal(cover, [len(w) for w in ws]), (name, sd, step)
        xs = r['x1'] + e[:, step]


@pytest.mark.parametrize('shift_rows', [None, '0'])
@pytest.mark.parametrize('sd', [0., 0.05])
@pytest.mark.parametrize('name', en.SMALL)
def test_host_shifted_covers_are_lower_bounds_of_the_next_problem(monkeypatch, name, sd, shift_rows):
    from warm_start_hmpc_amd.batched import BatchedMPC
    from warm_start_hmpc_amd.search import DeviceSearch
    if shift_rows is None:
        monkeypatch.delenv('HMPC_SHIFT_ROWS', raising=False)
    else:
        monkeypatch.setenv('HMPC_SHIFT_ROWS', shift_rows)
    ctrl, d = _search_backend(name)
    bm = BatchedMPC(ctrl)
    assert bm.device_shift
    xs = _loop_states(name)
    K = len(xs)
    e = _errors(d['nx'], sd, K)
    ds = DeviceSearch(ctrl, K, node_cap=2048, row_cap=K * 2048)
    ws, worst = None, en.Report('bounds')
    for step in range(STEPS):
        out = ds.feedforward_many(xs, ws, frontier_width=8, tol=0., handdown=True)
        _hold_many(name, xs, out, (name, sd, shift_rows, step))
        assert all(r['ub'] is not None for r in out)
        ws = bm.construct_warm_start_many([r['leaves'] for r in out], xs, np.array([np.concatenate((r['uc'][0], r['ub'][0])) for r in out]), e[:, step])
        xs = np.array([r['x'][1] for r in out]) + e[:, step]
        for k in range(K):
            worst.merge(en.hold_tree(_truth(name, xs[k]), ws[k].fix, ws[k].lb, (name, sd, shift_rows, step, k, 'warm start'), quarter=True))
    _hold_many(name, xs, ds.feedforward_many(xs, ws, frontier_width=8, tol=0., handdown=True), (name, sd, shift_rows, 'last'))
    _note('host shift (rows %s) sd %g' % (shift_rows, sd), worst)
    assert worst.finite > 0


def _hold_flat(name, xs, lv, what, quarter=True):
    worst = en.Report('bounds')
    for k in range(len(xs)):
        m = lv['owner'] == k
        worst.merge(en.hold_tree(_truth(name, xs[k]), lv['fix'][m], lv['lb'][m], (what, k), quarter=quarter))
    return worst


def _hold_results(name, xs, res, what):
    for k in range(len(xs)):
        t = _truth(name, xs[k])
        assert t.feasible and res['state'][k] == (sr.DONE | sr.INCUMBENT), (what, k, res['state'])
        en.hold(en.result(t, res['cost'][k], res['binaries'][k], res['u0'][k], res['x1'][k]), (what, k))


@pytest.mark.parametrize('sd', [0., 0.05])
@pytest.mark.parametrize('name', en.SMALL)
def test_advanced_covers_are_lower_bounds_of_the_next_problem(name, sd):
    from warm_start_hmpc_amd.batched import BatchedMPC
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, d = _search_backend(name)
    BatchedMPC(ctrl)                                                            # (the shift's maps)
    xs = _loop_states(name)
    K = len(xs)
    e = _errors(d['nx'], sd, K)
    ds = DeviceSearch(ctrl, K, node_cap=2048, row_cap=K * 2048)
    ds.begin(xs)
    worst = en.Report('bounds')
    for step in range(STEPS):
        ds.run(8, 0., True)
        res = ds.results()
        _hold_results(name, xs, res, (name, sd, step))
        _hold_flat(name, xs, ds.leaves_flat(), (name, sd, step, 'leaves'), quarter=False)
        a = ds.advance(e[:, step])
        xs = res['x1'] + e[:, step]
        lv = ds.leaves_flat()
        assert np.array_equal(np.bincount(lv['owner'], minlength=K), a['cover'])
        worst.merge(_hold_flat(name, xs, lv, (name, sd, step, 'advanced')))
    ds.run(8, 0., True)
    _hold_results(name, xs, ds.results(), (name, sd, 'last'))
    _note('advance sd %g' % sd, worst)
    assert worst.finite > 0


@pytest.mark.parametrize('sd', [0., 0.05])
@pytest.mark.parametrize('name', en.SMALL)
def test_rebased_trees_are_lower_bounds_of_the_measured_states_problem(name, sd):
    from warm_start_hmpc_amd.batched import BatchedMPC
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, d = _search_backend(name)
    BatchedMPC(ctrl)
    xs = _loop_states(name)
    K = len(xs)
    e = _errors(d['nx'], sd, K)
    ds = DeviceSearch(ctrl, K, node_cap=2048, row_cap=K * 2048)
    ds.begin(xs)
    ds.run(8, 0., True)
    based = en.Report('bounds')
    for step in range(STEPS):
        res = ds.results()
        _hold_results(name, xs, res, (name, sd, step))
        predicted = res['x1'].copy()
        ds.advance(None)                                                        # to the model's next state (the test above holds that cover)
        ds.run(8, 0., True)                                                     # the idle-time search
        xs = predicted + e[:, step]
        ds.rebase(xs)                                                           # to the measured one
        based.merge(_hold_flat(name, xs, ds.leaves_flat(), (name, sd, step, 're-based')))
        ds.run(8, 0., True)
    _hold_results(name, xs, ds.results(), (name, sd, 'last'))
    _note('rebase sd %g' % sd, based)
    assert based.finite > 0


# ---- anytime -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('budget', [1, 4, 16])
@pytest.mark.parametrize('rule', ['best', 'depth', 'breadth', 'dive'])
@pytest.mark.parametrize('name', en.SMALL)
def test_an_anytime_search_brackets_the_enumerated_optimum_at_every_stop(name, rule, budget):
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, d = _search_backend(name)
    x0s = en.states(name)
    K = len(x0s)
    ts = [_truth(name, x) for x in x0s]
    ds = DeviceSearch(ctrl, K, node_cap=8192, row_cap=K * 8192, rule=rule, max_solves=budget)
    ds.begin(x0s)
    worst = 0.
    for stop in range(4):
        ds.run(8, 0., False)
        b, res = ds.bounds(0.), ds.results()
        assert (res['solves'] <= (stop + 1) * budget).all()
        for k in range(K):
            got = en.hold(en.bracket(ts[k], b['lower'][k], b['upper'][k]), (name, rule, budget, stop, k))
            worst = max(worst, got.worst) if np.isfinite(got.worst) else worst
            assert ts[k].feasible or b['upper'][k] == np.inf, (name, rule, budget, stop, k)
        _hold_flat(name, x0s, ds.leaves_flat(), (name, rule, budget, stop), quarter=False)
        ds.set_budget((stop + 2) * budget)
    ds.set_budget(None)
    ds.run(8, 0., False)
    b, res = ds.bounds(0.), ds.results()
    assert np.all(res['state'] & sr.DONE) and not np.any(res['state'] & (sr.FAILED | sr.OVERFLOW | ar.BUDGET))
    for k in range(K):
        en.hold(en.result(ts[k], res['cost'][k], res['binaries'][k] if ts[k].feasible else None, res['u0'][k], res['x1'][k]), (name, rule, budget, 'done', k))
        en.hold(en.bracket(ts[k], b['lower'][k], b['upper'][k]), (name, rule, budget, 'done', k))
        assert ts[k].feasible or (b['upper'][k] == np.inf and b['lower'][k] == np.inf), (name, rule, budget, k, b['lower'][k])
    print(name, rule, budget, 'worst (lower - optimum) / (1 + optimum) at a stop: %.3g' % worst)
