"""Anytime device searches on the device (include/hmpc_search_anytime.h: the select, stage, reopen and bounds kernels of
csrc/hmpc_search.hip), held to the numpy restatement of tests/anytime_reference.py -- integers exactly, floats bit for bit -- on
synthetic rounds over the edges of the kernels and on whole cart-pole searches under every rule; a search that is never configured
against one configured to the defaults; budgets on real trees against the optimum of the unbudgeted search; a cut-off search
resumed; a cut-off tree carried into the next step; the refusals that need a handle."""
import numpy as np
import pytest

import anytime_reference as ar
import branch_reference as br
import search_reference as sr
import speculation_reference as sp
from test_gpu_branch import _backend
from test_gpu_search import SCAN_CHUNK, X0, _cover_arrays, _solver

pytestmark = pytest.mark.gpu
RTOL = 1e-5                # the suite's parity tolerance (tests/test_gpu_parity.py)
WIDE = np.array([-0.058, 0.016, 0.761, -0.326])    # a state near X0 whose tree holds more candidates than a round is wide
STATES = {'cart_pole_t16': np.array([X0 * .5, X0 * .4, X0]),      # (from X0 itself sixteen stages are infeasible: a search without incumbent)
          'cart_pole_t20': np.array([X0, X0 * .5, WIDE])}
# Test 10: rule dive at width 8, states and budgets chosen with the restatement over the oracle backend.  A budget cuts the LAST round of a
# tree short (a round stages min(width, max_solves - solves) picks, the deepest first under dive), so a tree is cut off WITH an
# incumbent where the budget ends between the solve that finds its first incumbent and its last solve:
#   t16: NARROW needs 179 solves there; m = 175 .. 178 leave it BUDGET | INCUMBENT with upper - lower = 0.0013 (X0 / 2: 129 solves,
#        DONE; X0: infeasible, DONE after 121)
#   t20: WIDE needs 407 solves and has its first incumbent at solve 355, with 6 candidates left and upper - lower = 0.0089
#        (X0: 161 solves, X0 / 2: 235)
#   64: every tree is cut off before it has an incumbent;  176 / 376: cut off WITH one, the others DONE;  256 / 512: all DONE.
NARROW = np.array([0.019606617477065727, -0.12279276789336097, 0.8986782928648392, -0.13273368455812876])
BUDGET_STATES = {'cart_pole_t16': np.array([X0 * .5, NARROW, X0]), 'cart_pole_t20': STATES['cart_pole_t20']}
BUDGETS = {'cart_pole_t16': (64, 176, 256), 'cart_pole_t20': (64, 376, 512)}
CUT_WITH_INCUMBENT = 376


def _search(name, K, node_cap, row_cap, **kw):
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, qp, d = _backend(name)
    return DeviceSearch(ctrl, K, node_cap=node_cap, row_cap=row_cap, **kw), d


def _tree_equal(a, b, what):
    """Two trees as DeviceSearch.tree returns them: every scalar, and the first n entries of every slab (entries beyond n are
    whatever the allocation held)."""
    assert a['n'] == b['n'], (what, 'n')
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert br.same_bits(x[:a['n']] if x.ndim else x, y[:a['n']] if y.ndim else y), (what, key)


# ---- 7. kernel edges -----------------------------------------------------------------------------------------------------------------
SIZES = lambda cap: (1, 63, 64, 65, cap - 2, cap - 1, 0)


@pytest.mark.parametrize('rule', [ar.BEST, ar.DEPTH, ar.BREADTH, ar.DIVE])
@pytest.mark.parametrize('width', [1, 8, 64])
@pytest.mark.parametrize('name,K', [('random_mld_t5', 1), ('random_mld_t5', 5), ('cart_pole_t16', 7), ('random_mld_t5', SCAN_CHUNK + 1)])
def test_synthetic_rounds_on_the_edges_of_the_kernels_under_rules_and_budgets(name, K, width, rule):
    # the layout of test_gpu_search.py's test of this name: trees of 1, 63, 64, 65, node_cap - 2, node_cap - 1 leaves and, in between,
    # trees without a leaf or with +inf bounds only; K = 1025: one tree past the offsets kernel's chunk.  Budgets 0 (no tree picks: a
    # round of nothing but stop words), 1 (a round of one pick per tree, then stop words) and width + 1 (a full round, one pick, stop)
    cap = 96
    ds, d = _search(name, K, cap, 3 * K * min(width, cap) + K * cap)
    ds.set_rule(rule)
    sizes = [SIZES(cap)[(k + (3 if K == 1 else 1)) % 7] for k in range(K)]
    watch = sorted(set(list(range(min(K, 7))) + list(range(0, K, 16)) + [K - 1]))   # every round; after a budget's last round EVERY tree
    for budget in (0, 1, width + 1):
        rng = np.random.default_rng(K * 100 + width + 7 * budget)
        covers = []
        for k, n in enumerate(sizes):
            f, l = sr.random_cover(d, n, rng)
            if k % 7 == 2 and k != K - 1:
                l[:] = np.inf
            covers.append((f, l, rng.uniform(0., 1., (n, d['n_dual'])), rng.uniform(0., 1., n)))
        ref = ar.Search(d, K, cap, ds.row_cap, rule=rule, max_solves=budget)
        x0s = rng.uniform(-1., 1., (K, d['nx']))
        ref.begin(x0s, covers)
        ds.begin(x0s, _cover_arrays(covers))
        ds.set_budget(budget)
        picks = []
        for q in range(3):
            what = (name, K, width, rule, budget, q)
            tol = .5 if q == 2 else 0.
            B = ref.select(width, tol, q % 2 == 0)
            assert ds.select(width, tol, q % 2 == 0) == B and ds._P == ref.P, what
            picks.append(ref.P)
            if B:
                sr.compare_dicts(ref.batch, ds.batch(), what=(what, 'batch'))
                rec = sr.synthetic_records(d, ref.batch['fix'], rng)
                ref.put_records(rec)
                ds.put_records(rec)
                ref.consume(tol)
                ds.consume(tol)
            for k in (watch if q < 2 else range(K)):
                sp.compare_tree(ref.tree(k), ds.tree(k), what=(what, 'tree', k))
            sr.compare_dicts(ref.results(), ds.results(), what=(what, 'results'))
            sr.compare_dicts(ref.bounds(tol), ds.bounds(tol), what=(what, 'bounds'))
        res = ref.results()
        assert (res['solves'] <= budget).all() and not np.isnan(ref.bounds(0.)['lower']).any()
        stopped = (res['state'] & ar.BUDGET) != 0
        assert (budget > 1 or stopped.any()) and (budget == 0 or picks[0] > 0)
        if budget == 0:
            assert picks == [0, 0, 0] and res['solves'].sum() == 0
        if K > SCAN_CHUNK:                                                      # the tree behind the carry (65 leaves) took part and got its word
            assert (budget > 1 or stopped[K - 1]) and (budget == 0 or res['solves'][K - 1] > 0)


# ---- 8. the default is untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('handdown', [False, True])
@pytest.mark.parametrize('width', [1, 8])
def test_a_search_configured_to_the_defaults_is_the_search_that_was_never_configured(width, handdown):
    a, d = _search('cart_pole_t16', 3, 512, 1024)
    b, _ = _search('cart_pole_t16', 3, 512, 1024)
    b.set_rule(0)
    b.set_budget(-1)
    x0s = STATES['cart_pole_t16']
    a.begin(x0s)
    b.begin(x0s)
    rounds = 0
    while True:
        ra, rb = a.run(width, 0., handdown, max_rounds=1), b.run(width, 0., handdown, max_rounds=1)      # (one launch per handle at a time)
        assert ra == rb
        if ra[0] == 0:
            break
        rounds += 1
        for k in range(3):
            _tree_equal(a.tree(k), b.tree(k), (width, handdown, rounds, k))
        row0 = a.batch()['row0']
        assert row0 == b.batch()['row0']
        pa, pb = a.rows(0, row0), b.rows(0, row0)
        for key in sr.RECORD_KEYS:
            assert br.same_bits(pa[key], pb[key]), (width, handdown, rounds, key)
    sr.compare_dicts(a.results(), b.results())
    assert rounds >= 16 and np.array_equal(a.results()['state'], [sr.DONE | sr.INCUMBENT] * 2 + [sr.DONE])
    assert br.same_bits(a.bounds()['lower'], b.bounds()['lower']) and np.array_equal(a.bounds()['open'], [0, 0, 0])


# ---- 9. whole searches ---------------------------------------------------------------------------------------------------------------
_BEST = {}


def _best_first(name):
    """The unbudgeted best-first search of the problem's three states: (results, trees)."""
    if name not in _BEST:
        ds, d = _search(name, 3, 2048, 8192)
        ds.begin(STATES[name])
        ds.run(8, 0., False)
        _BEST[name] = ds.results()
        assert not (_BEST[name]['state'] & (sr.FAILED | sr.OVERFLOW)).any()
    return _BEST[name]


@pytest.mark.parametrize('rule', ['depth', 'breadth', 'dive'])
@pytest.mark.parametrize('width', [1, 8])
@pytest.mark.parametrize('name', ['cart_pole_t16', 'cart_pole_t20'])
def test_cart_pole_searches_under_a_rule_match_the_restatement_to_the_bit(name, width, rule):
    ctrl, qp, d = _backend(name)
    x0s = STATES[name]
    ds, _ = _search(name, 3, 2048, 8192, rule=rule)
    ref = ar.Search(d, 3, 2048, 8192, rule=ar.RULES[rule])
    solve = _solver(qp, ref, False)
    ref.begin(x0s)
    ds.begin(x0s)
    rounds = 0
    while True:
        B = ref.select(width, 0., False)
        P = ref.P
        if P:
            ref.put_records(solve(ref.batch['x0'], ref.batch['fix'], ref.batch['warm']))
            ref.consume(0.)
        assert ds.run(width, 0., False, max_rounds=1) == ((1, B) if P else (0, 0)), (name, width, rule, rounds)
        sr.compare_dicts(ref.results(), ds.results(), what=(name, width, rule, 'round', rounds))
        sr.compare_dicts(ref.bounds(0.), ds.bounds(0.), what=(name, width, rule, 'bounds', rounds))
        if rounds % 16 == 0 or not P:
            for k in range(3):
                sp.compare_tree(ref.tree(k), ds.tree(k), what=(name, width, rule, 'round', rounds, 'tree', k))
        if not P:
            break
        rounds += 1
    sr.compare_dicts(ref.leaves(), ds.leaves_flat(), what=(name, width, rule, 'leaves'))
    got, best = ds.results(), _best_first(name)
    print('%s width %d %s: %d rounds, solves %s (best-first %s), cost %s' % (name, width, rule, rounds, got['solves'], best['solves'], got['cost']))
    assert np.all(got['state'] & sr.DONE) and not np.any(got['state'] & (sr.FAILED | sr.OVERFLOW | ar.BUDGET))
    fin = np.isfinite(best['cost'])
    assert np.array_equal(fin, np.isfinite(got['cost'])) and fin.sum() >= 2
    np.testing.assert_allclose(got['cost'][fin], best['cost'][fin], rtol=RTOL, atol=0.)
    assert np.array_equal(got['binaries'], best['binaries'])


def test_speculation_under_depth_first_is_depth_zero_in_everything_but_row_numbers():
    name, width = 'cart_pole_t16', 8
    x0s = STATES[name]
    flat, _ = _search(name, 3, 1024, 4096, rule='depth')
    deep, _ = _search(name, 3, 1024, 7 * 4096, rule='depth', speculation=2)
    flat.begin(x0s)
    deep.begin(x0s)
    flat.run(width, 0., False)
    deep.run(width, 0., False)
    sr.compare_dicts(flat.results(), deep.results())
    ca, cb = flat.counters(), deep.counters()
    assert cb['launches'] < ca['launches'] and cb['rounds'] == ca['rounds'] and cb['served'] > 0
    pa, pb = flat.rows(0, flat.batch()['row0']), deep.rows(0, deep.batch()['row0'])
    for k in range(3):
        sp.compare_modulo_rows(flat.tree(k), deep.tree(k), pa, pb, what=k)


def test_feedforward_many_takes_the_selection_functions_of_the_host_driver():
    # the reference's candidate_selection argument on this path: the same solves, the same optimum and as many leaves as
    # controller.feedforward(search_rule=...) -- branch_and_bound on the host -- finds through the same handle
    from warm_start_hmpc_amd import branch_and_bound as bb
    ctrl, qp, d = _backend('cart_pole_t20')
    x0s = STATES['cart_pole_t20']
    ds, _ = _search('cart_pole_t20', 3, 2048, 8192)
    for selection, name in ((bb.depth_first, 'depth'), (bb.breadth_first, 'breadth'), (bb.best_first, 'best')):
        out = ds.feedforward_many(x0s, None, frontier_width=8, handdown=False, search_rule=selection)
        assert ds.rule == name
        for k in range(3):
            sol, leaves, solves, _ = ctrl.feedforward(x0s[k], search_rule=selection, frontier_width=8, printing_period=None, handdown=False)
            assert out[k]['solves'] == solves and len(out[k]['leaves']) == len(leaves), (name, k, out[k]['solves'], solves)
            np.testing.assert_allclose(out[k]['objective'], sol.objective, rtol=RTOL, atol=0.)
    with pytest.raises(ValueError, match='selection function'):
        ds.set_rule(lambda candidates: candidates[len(candidates) // 2])
    assert ds.rule == 'best'


# ---- 10. budgets on real trees -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cart_pole_t16', 'cart_pole_t20'])
def test_budgets_stop_real_trees_with_bounds_that_bracket_the_optimum(name):
    x0s = BUDGET_STATES[name]
    ds, d = _search(name, 3, 2048, 8192)
    ds.begin(x0s)
    ds.run(8, 0., False)                                                        # the unbudgeted search of the same states on the same handle
    full = ds.results()
    assert np.all(full['state'] & sr.DONE) and not np.any(full['state'] & (sr.FAILED | sr.OVERFLOW))
    opt = full['cost']
    ds.set_rule('dive')
    cut_with = cut_without = done = 0
    for m in BUDGETS[name]:
        ds.set_budget(m)
        ds.begin(x0s)
        ds.run(8, 0., False)
        r, b = ds.results(), ds.bounds(0.)
        print('%s m = %d: state %s solves %s lower %s upper %s open %s (optimum %s)' % (name, m, r['state'], r['solves'], b['lower'], b['upper'], b['open'], opt))
        assert (r['solves'] <= m).all()
        assert all(s in (sr.DONE, sr.DONE | sr.INCUMBENT, ar.BUDGET, ar.BUDGET | sr.INCUMBENT) for s in r['state'])
        slack = np.where(np.isfinite(opt), RTOL * np.maximum(1., np.abs(opt)), 0.)     # (an infeasible MIQP: lower <= inf, upper == inf)
        assert not np.isnan(b['lower']).any()
        assert (b['lower'] <= opt + slack).all() and (b['upper'] >= opt - slack).all()
        assert br.same_bits(b['upper'], np.where(r['state'] & sr.INCUMBENT, r['cost'], np.inf))
        assert np.array_equal(b['open'] > 0, (r['state'] & ar.BUDGET) != 0)
        cut = (r['state'] & ar.BUDGET) != 0
        has = (r['state'] & sr.INCUMBENT) != 0
        cut_with += int((cut & has & (b['upper'] > b['lower'])).sum())                # (upper - lower > 0, without inf - inf)
        cut_without += int((cut & ~has).sum())
        done += int(((r['state'] & sr.DONE) != 0).sum())
    assert cut_with > 0 and cut_without > 0 and done > 0


# ---- 11. resume ----------------------------------------------------------------------------------------------------------------------
def test_a_cut_off_search_resumed_without_budget_is_the_unbudgeted_search():
    name = 'cart_pole_t16'
    x0s = STATES[name][:2]
    one, d = _search(name, 2, 512, 1024)
    two, _ = _search(name, 2, 512, 1024)
    one.begin(x0s)
    one.run(1, 0., False)
    two.set_budget(40)
    two.begin(x0s)
    two.run(1, 0., False)
    cut = two.results()
    assert np.array_equal(cut['state'], [ar.BUDGET] * 2) and np.array_equal(cut['solves'], [40, 40]) and np.array_equal(two.bounds()['open'] > 0, [True] * 2)
    two.set_budget(-1)
    two.run(1, 0., False)
    # width 1: every round has exactly one pick per running tree, so the walk is the same -- trees and pool to the bit
    sr.compare_dicts(one.results(), two.results())
    assert np.array_equal(one.results()['state'], [sr.DONE | sr.INCUMBENT] * 2)
    for k in range(2):
        _tree_equal(one.tree(k), two.tree(k), k)
    row0 = one.batch()['row0']
    assert row0 == two.batch()['row0'] == int(one.results()['solves'].sum())
    pa, pb = one.rows(0, row0), two.rows(0, row0)
    for key in sr.RECORD_KEYS:
        assert br.same_bits(pa[key], pb[key]), key
    # width 8: a budget cuts rounds short, so the walks differ; what they find does not
    wide, _ = _search(name, 2, 512, 1024, max_solves=40)
    wide.begin(x0s)
    wide.run(8, 0., False)
    assert np.all(wide.results()['state'] & ar.BUDGET)
    wide.set_budget(None)
    wide.run(8, 0., False)
    r = wide.results()
    assert np.array_equal(r['state'], [sr.DONE | sr.INCUMBENT] * 2) and np.array_equal(r['binaries'], one.results()['binaries'])
    np.testing.assert_allclose(r['cost'], one.results()['cost'], rtol=RTOL, atol=0.)


# ---- 12. a cut-off tree advances -----------------------------------------------------------------------------------------------------
def _is_cover(fix):
    """Leaves with prefix identifiers cover the binary cube exactly once iff sum 2^(free binaries) == 2^nfix (Python integers)."""
    nfix = fix.shape[1]
    return sum(2 ** int((f < 0).sum()) for f in fix) == 2 ** nfix


def test_a_tree_cut_off_with_an_incumbent_advances_and_its_leaves_still_cover_the_cube():
    from helpers import load_fixture
    from warm_start_hmpc_amd.batched import BatchedMPC
    name, K, steps, m = 'cart_pole_t20', 3, 3, CUT_WITH_INCUMBENT
    ctrl, qp, d = _backend(name)
    x0s = STATES[name]
    errors = load_fixture('reference_closed_loop')['errors_0003'][:K, :steps]
    # the loop without a budget is the resident loop as it was
    plain = _search(name, K, 2048, 8192)[0].closed_loop(x0s, steps, errors, frontier_width=8, handdown=False, resident=True)
    same = _search(name, K, 2048, 8192)[0].closed_loop(x0s, steps, errors, frontier_width=8, handdown=False, resident=True, rule='best', max_solves=-1)
    for key in ('nodes_ws', 'len_ws', 'reopened', 'costs', 'steps'):
        assert br.same_bits(np.asarray(plain[key]), np.asarray(same[key])), key
    assert not same['stopped'].any() and (same['lower'] <= same['costs'])[np.isfinite(same['costs'])].all()
    # the loop under a budget
    loop = _search(name, K, 2048, 8192, rule='breadth')[0]
    stats = loop.closed_loop(x0s, steps, errors, frontier_width=8, handdown=False, resident=True, rule='dive', max_solves=m)
    assert loop.rule == 'breadth' and loop.max_solves is None                   # the loop's rule and budget do not outlive it
    loop.begin(x0s)
    loop.run(8, 0., False)
    assert np.all(loop.results()['state'] & sr.DONE) and (loop.results()['solves'] > m).any()
    print('stopped %s\nsolves %s\ncosts %s\nlower %s' % (stats['stopped'].tolist(), stats['nodes_ws'].tolist(), stats['costs'].tolist(), stats['lower'].tolist()))
    assert stats['stopped'][:, 0].any() and np.isfinite(stats['costs'][stats['stopped'][:, 0], 0]).all()   # cut off WITH an incumbent: it advanced
    assert (stats['len_ws'][:, 0] > 0).all() and stats['steps'] >= K and (stats['nodes_ws'] <= m).all()
    both = np.isfinite(stats['lower']) & np.isfinite(stats['costs'])
    assert both.any() and (stats['lower'][both] <= stats['costs'][both]).all()
    # the step boundary by hand: the cut-off tree is accepted, its leaves cover the cube, and every bound of the new step is one
    BatchedMPC(ctrl)                                                            # (the shift's maps)
    ds, _ = _search(name, K, 2048, 8192, rule='dive', max_solves=m)
    ds.begin(x0s)
    ds.run(8, 0., False)
    r = ds.results()
    assert r['state'][2] == ar.BUDGET | sr.INCUMBENT and np.all(r['state'] & sr.INCUMBENT)
    a = ds.advance(errors[:, 0])
    assert (a['cover'] > 0).all() and np.array_equal(ds.results()['state'], [0] * K) and np.array_equal(ds.results()['solves'], [0] * K)
    lv = ds.leaves_flat()
    x_next = r['x1'] + errors[:, 0]
    cold, _ = _search(name, K, 2048, 8192)
    cold.begin(x_next)
    cold.run(8, 0., False)
    nxt = cold.results()
    assert np.all(nxt['state'] & sr.DONE) and not np.any(nxt['state'] & (sr.FAILED | sr.OVERFLOW))
    low = ds.bounds()['lower']
    for k in range(K):
        mine = lv['owner'] == k
        fix, lb = lv['fix'][mine], lv['lb'][mine]
        assert mine.sum() == a['cover'][k] and _is_cover(fix), k
        # Every leaf's bound is a dual bound of ITS part of the cube.  Leaves the old step pruned or proved infeasible carry bounds
        # above the new optimum (or +inf), so the bound is held to the optimum where the optimum lies: the one leaf that contains
        # the cold search's optimal binaries, and with it the minimum over the cover (what `bounds` reports as lower)
        bound = nxt['cost'][k] + RTOL * max(1., abs(nxt['cost'][k]))
        holds = [j for j in range(len(fix)) if np.array_equal(fix[j][fix[j] >= 0], nxt['binaries'][k][fix[j] >= 0])]
        assert len(holds) == 1 and not np.isnan(lb).any(), (k, holds)
        print('tree %d: cover %d (reopened %d), lower %.6f, bound of the leaf that holds the optimum %.6f, next optimum %.6f, leaves bounded above it %d'
              % (k, a['cover'][k], a['reopened'][k], low[k], lb[holds[0]], nxt['cost'][k], int((lb > bound).sum())))
        assert lb[holds[0]] <= bound and low[k] <= bound and low[k] == lb.min(), (k, lb[holds[0]], low[k], nxt['cost'][k])


# ---- 13. refusals that need a handle -------------------------------------------------------------------------------------------------
def test_configuration_and_bounds_are_refused_while_a_round_is_staged_and_a_refused_round_writes_no_stop_word():
    from warm_start_hmpc_amd.search import SearchTooBig
    ds, d = _search('random_mld_t5', 2, 32, 64)
    lib = ds.qp.lib
    out = np.full(2, -7.)
    assert lib.hmpc_search_bounds(ds._s, 0., out.ctypes.data, None, None, None) == -1 and b'no step has begun' in lib.hmpc_last_error()
    rng = np.random.default_rng(3)
    covers = []
    for n in (5, 9):
        f, l = sr.random_cover(d, n, rng, ties=False, infs=False)
        covers.append((f, l, rng.uniform(0., 1., (n, d['n_dual'])), rng.uniform(0., 1., n)))
    ds.begin(np.zeros((2, d['nx'])), _cover_arrays(covers))
    assert ds.select(4, 0., True) == 8
    before = [ds.tree(k) for k in range(2)]
    assert lib.hmpc_search_set_rule(ds._s, 1) == -1 and b'staged' in lib.hmpc_last_error()
    assert lib.hmpc_search_set_budget(ds._s, 3, None) == -1 and b'staged' in lib.hmpc_last_error()
    assert lib.hmpc_search_bounds(ds._s, 0., out.ctypes.data, None, None, None) == -1 and b'staged' in lib.hmpc_last_error() and (out == -7.).all()
    for bad, call in ((ValueError, lambda: ds.set_rule('depth')), (ValueError, lambda: ds.set_budget(3)), (ValueError, ds.bounds)):
        with pytest.raises(bad):
            call()
    with pytest.raises(ValueError):
        ds.set_rule('deepest')
    for k in range(2):
        _tree_equal(before[k], ds.tree(k), ('staged', k))
    assert ds.rule == 'best' and ds.max_solves is None
    # the staged round is still the round: it is consumed as if nothing had been asked
    rec = sr.synthetic_records(d, ds.batch()['fix'], rng)
    ds.put_records(rec)
    ds.consume(0.)
    assert np.array_equal(ds.results()['solves'], [4, 4])
    # a round refused for row_cap under an exhausted budget.  Budget 4 at width 4: tree 0 has ONE candidate, whose record branches;
    # tree 1 spends its budget in round 0.  Round 1 would pick tree 0's two children and stop tree 1 -- in a pool one row short it
    # is refused, and tree 1's word stays 0; in a pool that holds it the same round writes the word
    covers[0][1][1:] = np.inf
    covers[0][0][0, 1:] = -1
    for row_cap, fits in ((14 + 5 + 1, False), (14 + 5 + 2, True)):
        ds, _ = _search('random_mld_t5', 2, 32, row_cap, max_solves=4)
        ds.begin(np.zeros((2, d['nx'])), _cover_arrays(covers))
        assert ds.select(4, 0., True) == 5 and list(ds.batch()['tree']) == [0, 1, 1, 1, 1]
        ds.put_records(sr.synthetic_records(d, ds.batch()['fix'], np.random.default_rng(8), plan={0: (0, .25, br.POLISHED_BIT | 3)}))
        ds.consume(0.)
        before = [ds.tree(k) for k in range(2)]
        assert [t['state'] for t in before] == [0, 0] and [t['solves'] for t in before] == [1, 4] and before[0]['n'] == 7
        if fits:
            assert ds.select(4, 0., True) == 2 and list(ds.results()['state'] & ~sr.INCUMBENT) == [0, ar.BUDGET]
            continue
        with pytest.raises(SearchTooBig, match='row_cap'):
            ds.select(4, 0., True)
        for k in range(2):
            _tree_equal(before[k], ds.tree(k), ('refused', k))
        assert list(ds.results()['state']) == [0, 0] and ds.bounds()['open'][1] > 0
