"""Every search path that runs without a GPU -- branch_and_bound under its three rules, BatchedMPC, and the numpy restatements the
device searches are compared with -- held to the exhaustively enumerated optimum of tests/enumeration_reference.py on the CPU
oracle: the optimum, the incumbent's binaries, u0 and x1; every final leaf's bound against the minimum of the leaves below it;
the leaves as a partition of the cube; and, across step boundaries of closed loops, every shifted, advanced or re-based bound
against the enumeration of the NEXT state's problem.  First the enumeration itself is held to the dense active-set solve and to
the certificates, which share no code with the oracle; last, the checkers are shown to refuse six planted defects."""
import numpy as np
import pytest

import advance_reference as adv
import anytime_reference as ar
import branch_reference as br
import enumeration_reference as en
import rebase_reference as rr
import search_reference as sr
from warm_start_hmpc_amd import branch_and_bound as bb

RULES = {'best': bb.best_first, 'depth': bb.depth_first, 'breadth': bb.breadth_first}
RICH = dict(handdown=True, speculation_depth=2, frontier_width=8, tol=0.05)
_CTRL = {}


def ctrl_of(name, threads=8):
    """One controller per workload on an oracle of eight threads -- and one on a single thread for the searches that solve a node at a
    time (the truths are shared: enumeration_reference caches them per problem, not per controller)."""
    if (name, threads) not in _CTRL:
        _CTRL[name, threads] = en.controller(name, threads=threads)
    return _CTRL[name, threads]


def _solve_with(ctrl):
    return lambda x0b, fix, warm: br.as_word_records(ctrl.qp.solve_batch(x0b, fix))


def _fix_of(ctrl, leaves):
    return np.array([ctrl._fix_vector(l.identifier) for l in leaves], np.int8).reshape(len(leaves), ctrl.T * ctrl.mld.nub)


# ---- the truth is trustworthy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', en.WORKLOADS)
def test_the_enumeration_is_held_to_the_dense_solve_and_the_certificates(name):
    from dense_qp import dense_qp, active_set_primal
    from certificates import assert_certified
    ctrl = ctrl_of(name)
    dq = dense_qp(ctrl)
    nxs = (ctrl.T + 1) * ctrl.mld.nx
    leaves = en.all_leaves(ctrl.T * ctrl.mld.nub)
    feasible = []
    xs = en.states(name)
    share = -(-64 // len(xs))                                                   # a seeded sample of 64 per workload, spread over its states
    for s, x0 in enumerate(xs):
        t = en.truth(ctrl, x0)
        rec = t.rec
        feasible.append(t.n_feasible)
        en.assert_gap(t, (name, s))
        rng = np.random.default_rng(100 + s)
        opt, inf = np.flatnonzero(rec['status'] == 0), np.flatnonzero(rec['status'] == 1)
        worst = 0.
        for i in (opt if opt.size <= share else rng.choice(opt, share, replace=False)):
            assert rec['polished'][i] > 0, (name, s, i)                          # a vertex: the active set of its multipliers is THE active set
            w, resid = active_set_primal(ctrl, dq, x0, leaves[i], rec['dual'][i])
            assert resid < 1e-9, (name, s, i, resid)
            dev = np.max(np.abs(w[:nxs] - rec['primal'][i][:nxs])) / max(1e-2, np.max(np.abs(w[:nxs])))
            worst = max(worst, dev)
            assert dev < 1e-7, ('dense active-set solve', name, s, int(i), dev)   # (the bound of tests/test_gpu_parity.py::_dense_check)
        pick = np.sort(np.concatenate((inf if inf.size <= share else rng.choice(inf, share, replace=False), [t.argmin] if t.feasible else [])).astype(np.int64))
        counts = assert_certified(ctrl, x0, leaves[pick], {k: rec[k][pick] for k in ('obj', 'dual_obj', 'status', 'primal', 'dual', 'polished', 'weak')},
                                  what='%s state %d' % (name, s))
        print('%s state %d: %d feasible leaves of %d, gap %.3g, dense solve within %.2e, certified %s' % (name, s, t.n_feasible, len(leaves), t.gap, worst, counts))
    if name in en.CART_POLES:
        # one leaf: the pole swings left of the wall it starts near and nothing else is consistent with the big-M rows;
        # with the terminal set the state (0, 0, 1, 0) cannot be brought home in three steps at all
        assert feasible == ([1, 0] if en.CART_POLES[name] else [1, 1]), feasible
        return
    dead = [s in en.MLDS[name][2] for s in en.MLDS[name][1]]
    assert all((n == 0) if d else (n >= 10) for n, d in zip(feasible, dead)), (name, feasible)


# ---- searches on the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['plain', 'rich'])
@pytest.mark.parametrize('rule', list(RULES))
@pytest.mark.parametrize('name', en.WORKLOADS)
def test_branch_and_bound_finds_the_enumerated_optimum_and_leaves_true_bounds(name, rule, variant):
    ctrl = ctrl_of(name, threads=1 if variant == 'plain' else 8)
    kw = RICH if variant == 'rich' else {}
    worst = en.Report('bounds')
    xs = en.states(name)
    for s, x0 in enumerate(xs if variant == 'rich' or len(xs) < 5 else xs[[1, 3, 4]]):      # (a node at a time: the nominal state, the one with the fewest feasible leaves, the last)
        t = en.truth(ctrl_of(name), x0)
        sol, leaves, solves, _ = ctrl.feedforward(x0, search_rule=RULES[rule], printing_period=None, **kw)
        what = (name, rule, variant, s)
        if sol is None:
            en.hold(en.result(t, np.inf, None), what)
        else:
            v = sol.variables
            en.hold(en.result(t, sol.objective, v['ub'], np.concatenate((v['uc'][0], v['ub'][0])), v['x'][1], tol=kw.get('tol', 0.)), what)
        worst.merge(en.hold_tree(t, _fix_of(ctrl, leaves), [l.lb for l in leaves], what))
    print(name, rule, variant, worst.figures())


@pytest.mark.parametrize('name', en.WORKLOADS)
def test_the_numpy_driver_finds_the_enumerated_optima_of_all_states_in_lockstep(name):
    from warm_start_hmpc_amd.batched import BatchedMPC
    ctrl = ctrl_of(name)
    x0s = en.states(name)
    out = BatchedMPC(ctrl).feedforward_many(x0s, None, frontier_width=8)
    worst = en.Report('bounds')
    for k, r in enumerate(out):
        t = en.truth(ctrl, x0s[k])
        if r['ub'] is None:
            en.hold(en.result(t, r['objective'], None), (name, k))
        else:
            en.hold(en.result(t, r['objective'], r['ub'], np.concatenate((r['uc'][0], r['ub'][0])), r['x'][1]), (name, k))
        worst.merge(en.hold_tree(t, r['leaves'].fix, r['leaves'].lb, (name, k)))
    print(name, worst.figures())


@pytest.mark.parametrize('budget', [1, 4, 16])
@pytest.mark.parametrize('rule', [ar.BEST, ar.DEPTH, ar.BREADTH, ar.DIVE])
@pytest.mark.parametrize('name', en.SMALL)
def test_the_anytime_restatement_brackets_the_optimum_at_every_stop(name, rule, budget):
    ctrl = ctrl_of(name)
    d = br.dims_of(ctrl.problem_data())
    x0s = en.states(name)[[1, 4]]                                               # the nominal state and the last (two of the problems: no feasible leaf)
    K = len(x0s)
    ts = [en.truth(ctrl, x) for x in x0s]
    ref = ar.Search(d, K, 8192, 16384, spec=0, rule=rule, max_solves=budget)     # (a tree of 2^12 leaves has 8191 nodes)
    ref.begin(x0s)
    solve = _solve_with(ctrl)
    for stop in range(3):
        ref.run(solve, 8, 0., False)
        b, lv = ref.bounds(0.), ref.leaves()
        for k in range(K):
            en.hold(en.bracket(ts[k], b['lower'][k], b['upper'][k]), (name, rule, budget, stop, k))
            m = lv['owner'] == k
            en.hold_tree(ts[k], lv['fix'][m], lv['lb'][m], (name, rule, budget, stop, k))
            if not ts[k].feasible:
                assert b['upper'][k] == np.inf
        ref.set_budget((stop + 2) * budget)
    ref.set_budget(-1)
    ref.run(solve, 8, 0., False)
    res, b = ref.results(), ref.bounds(0.)
    assert np.all(res['state'] & sr.DONE)
    for k in range(K):
        en.hold(en.result(ts[k], res['cost'][k], res['binaries'][k] if ts[k].feasible else None, res['u0'][k], res['x1'][k]), (name, rule, budget, 'done', k))
        assert ts[k].feasible or b['lower'][k] == np.inf


# ---- closed loops on the oracle ------------------------------------------------------------------------------------------------------
STEPS = 3


def _errors(nx, sd, K=1):
    return sd * np.random.default_rng(7).standard_normal((K, STEPS, nx))


def numpy_shift(bm, search):
    """The shift between stage and adopt of advance_reference.Search.advance: BatchedMPC.construct_warm_start, tree by tree."""
    from warm_start_hmpc_amd.batched import NodeArrays

    def shift(st):
        d, cap = search.d, search.row_cap
        B = len(st['owner'])
        out = dict(fix_out=np.zeros((B, d['nfix']), np.int8), lb_out=np.zeros(B), flags=np.zeros(B, np.uint8), dual=np.zeros((B, d['n_dual'])), dual_obj=np.zeros(B))
        for k in np.unique(st['owner']):
            m = np.flatnonzero(st['owner'] == k)
            has = st['src'][m] < cap
            rows = np.where(has, st['src'][m], 0)
            lv = NodeArrays(st['fix'][m], st['lb'][m].copy(), np.where(has[:, None], search.pool['dual'][rows], 0.), np.where(has, search.pool['dual_obj'][rows], 0.), has)
            u0 = st['u0'][k]
            ws = bm.construct_warm_start(lv, st['x0'][k], u0[:bm.nuc], u0[bm.nuc:], st['e0'][k])
            assert len(ws) == len(m)                                            # (retain has dropped what the shift would drop)
            out['fix_out'][m], out['lb_out'][m], out['dual'][m], out['dual_obj'][m] = ws.fix, ws.lb, ws.dual, ws.dobj
            out['flags'][m] = 1 | 2 * (has & ~ws.has_dual)
        return out
    return shift


@pytest.mark.parametrize('sd', [0., 0.05])
@pytest.mark.parametrize('name', en.SMALL)
def test_warm_starts_of_the_numpy_driver_are_lower_bounds_of_the_next_problem(name, sd):
    from warm_start_hmpc_amd.batched import BatchedMPC
    ctrl = ctrl_of(name)
    bm = BatchedMPC(ctrl)
    x, ws = en.states(name, infeasible=False)[1], None
    e = _errors(ctrl.mld.nx, sd)[0]
    worst, steps = en.Report('bounds'), 0
    for step in range(STEPS):
        t = en.truth(ctrl, x)
        en.assert_gap(t, (name, sd, step))
        r = bm.feedforward_many(x[None], [ws], frontier_width=8)[0]
        if not t.feasible:
            en.hold(en.result(t, r['objective'], None), (name, sd, step))
            break
        en.hold(en.result(t, r['objective'], r['ub'], np.concatenate((r['uc'][0], r['ub'][0])), r['x'][1]), (name, sd, step))
        en.hold_tree(t, r['leaves'].fix, r['leaves'].lb, (name, sd, step, 'leaves'))
        ws = bm.construct_warm_start(r['leaves'], x, r['uc'][0], r['ub'][0], e[step])
        x = r['x'][1] + e[step]
        worst.merge(en.hold_tree(en.truth(ctrl, x), ws.fix, ws.lb, (name, sd, step, 'warm start'), quarter=True))
        steps += 1
    print(name, sd, '%d boundaries;' % steps, worst.figures())
    assert steps == STEPS and worst.finite > 0


@pytest.mark.parametrize('sd', [0., 0.05])
@pytest.mark.parametrize('name', en.SMALL)
def test_advanced_and_rebased_trees_of_the_restatements_are_lower_bounds_of_the_next_problem(name, sd):
    # search_reference.Search (the base class: select / consume / results / leaves), advance_reference (retain -> shift -> adopt)
    # and rebase_reference (the bounds moved to a measured state), solved on the oracle: advance to the PREDICTED state, search
    # there, re-base to the measured one, search again -- the walk of DeviceSearch's presolve loop
    from warm_start_hmpc_amd.batched import BatchedMPC
    ctrl = ctrl_of(name)
    d = br.dims_of(ctrl.problem_data())
    bm = BatchedMPC(ctrl)
    ref = rr.Search(d, 1, 1024, 8192)
    shift, solve = numpy_shift(bm, ref), _solve_with(ctrl)
    x = en.states(name, infeasible=False)[1]
    e = _errors(ctrl.mld.nx, sd)[0]
    moved, based = en.Report('bounds'), en.Report('bounds')
    ref.begin(x[None])
    for step in range(STEPS):
        ref.run(solve, 8, 0., True)
        res, lv, t = ref.results(), ref.leaves(), en.truth(ctrl, x)
        assert res['state'][0] == adv.ADVANCES, (name, sd, step, res['state'])
        en.hold(en.result(t, res['cost'][0], res['binaries'][0], res['u0'][0], res['x1'][0]), (name, sd, step))
        en.hold_tree(t, lv['fix'], lv['lb'], (name, sd, step, 'leaves'))
        predicted = res['x1'][0].copy()
        ref.advance(shift)                                                      # (no error: the model's next state)
        lv = ref.leaves()
        moved.merge(en.hold_tree(en.truth(ctrl, predicted), lv['fix'], lv['lb'], (name, sd, step, 'advanced'), quarter=True))
        ref.run(solve, 8, 0., True)                                             # the idle-time search
        x = predicted + e[step]
        ref.rebase(x[None])
        lv = ref.leaves()
        based.merge(en.hold_tree(en.truth(ctrl, x), lv['fix'], lv['lb'], (name, sd, step, 're-based'), quarter=True))
    ref.run(solve, 8, 0., True)
    res = ref.results()
    en.hold(en.result(en.truth(ctrl, x), res['cost'][0], res['binaries'][0], res['u0'][0], res['x1'][0]), (name, sd, 'last'))
    print(name, sd, 'advanced:', moved.figures(), '| re-based:', based.figures())
    assert moved.finite > 0 and based.finite > 0


# ---- the checkers refuse planted defects ---------------------------------------------------------------------------------------------
def _a_warm_start():
    """A real warm start whose bounds are tight: mld_4_2_1_t12 after one step without model error.  (warm start, truth at the next state)."""
    from warm_start_hmpc_amd.batched import BatchedMPC
    ctrl = ctrl_of('mld_4_2_1_t12')
    bm = BatchedMPC(ctrl)
    x = en.states('mld_4_2_1_t12', infeasible=False)[1]
    r = bm.feedforward_many(x[None], None, frontier_width=8)[0]
    ws = bm.construct_warm_start(r['leaves'], x, r['uc'][0], r['ub'][0], np.zeros(ctrl.mld.nx))
    return ws, en.truth(ctrl, r['x'][1])


DEFECTS = {'raised_bound': 'bound', 'pruned_feasible': 'pruned_feasible', 'second_best': 'binaries', 'broken_cover': 'missing',
           'u0_of_stage_one': 'u0', 'lower_above': 'lower'}


@pytest.mark.parametrize('defect', list(DEFECTS))
def test_the_checkers_name_every_planted_defect(defect):
    ws, t = _a_warm_start()
    fix, lb = ws.fix.copy(), ws.lb.copy()
    holds = [j for j in range(len(lb)) if en.members(fix[j], t.nfix)[t.argmin]]
    assert len(holds) == 1 and en.bounds(t, fix, lb).ok and en.cover(fix).ok
    x, u = t.row(t.argmin)
    if defect == 'raised_bound':                                                # a warm-start bound 1e-4 (relative) too high
        j = holds[0]
        assert np.isfinite(lb[j]) and t.below(fix[j]) - lb[j] < 1e-5 * abs(lb[j])      # (the bound was tight: the defect is not hidden in slack)
        lb[j] *= 1. + 1e-4
        got = en.bounds(t, fix, lb)
    elif defect == 'pruned_feasible':                                           # +inf on the node the optimum lies below
        lb[holds[0]] = np.inf
        got = en.bounds(t, fix, lb)
    elif defect == 'second_best':                                               # the answer of a search that cut the optimum off
        second = int(np.argsort(t.obj, kind='stable')[1])
        xs, us = t.row(second)
        got = en.result(t, t.obj[second], en.all_leaves(t.nfix)[second], us[0], xs[1])
        assert 'cost' in got.names()
    elif defect == 'broken_cover':                                              # one leaf twice, one not at all (the volume is right)
        j = holds[0]
        both = np.repeat(fix[j][None], 2, axis=0)                               # the node of the optimum split on its first free binary ...
        k = int(np.flatnonzero(fix[j] < 0)[0])
        both[:, k] = (0, 1)
        rest = np.flatnonzero(both[0] < 0)
        both[:, rest] = 0                                                       # ... down to two leaves, and the rest of the node's part in between
        between = []
        for v in (0, 1):
            for q in range(len(rest)):
                node = both[v].copy()
                node[rest[q]] = 1
                node[rest[q + 1:]] = -1
                between.append(node)
        whole = np.concatenate((np.delete(fix, j, axis=0), both, np.array(between, np.int8).reshape(-1, t.nfix)))
        assert en.cover(whole).ok
        whole[len(fix) - 1] = whole[len(fix)]                                   # leaf (k = 0, rest 0) is gone, leaf (k = 1, rest 0) is there twice
        got = en.cover(whole)
        assert 'duplicated' in got.names() and 'volume' not in got.names()
    elif defect == 'u0_of_stage_one':
        assert en._close(u[1], u[0]) > 100 * en.RTOL
        got = en.result(t, t.best, en.all_leaves(t.nfix)[t.argmin], u[1], x[1])
    else:                                                                       # a proved lower bound above the optimum
        got = en.bracket(t, t.best * (1. + 1e-4) + 1e-8, np.inf)
    assert not got.ok and DEFECTS[defect] in got.names() and DEFECTS[defect] in got.report(), (defect, got.report())
