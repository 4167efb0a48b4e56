"""Anytime device searches (include/hmpc_search_anytime.h: node rules, solve budgets, proven bounds) without a GPU: the numpy
restatement of tests/anytime_reference.py held to its base class where nothing is configured and to the host driver's
branch_and_bound under depth_first / breadth_first on the oracle backend; the per-tree functions of csrc/hmpc_search.h -- what the
kernels run -- walked serially (tests/host/anytime_driver.cpp) under AddressSanitizer and UBSan and held to the restatement (integers
exactly, floats bit for bit) over all rules, widths, budgets and tree sizes; three planted defects, each of which the comparison
must catch; the new header against the binding; the refusals that need no GPU."""
import os
import re

import numpy as np
import pytest

import anytime_reference as ar
import branch_reference as br
import search_reference as sr
import speculation_reference as sp
from test_search_host import SHAPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def no_error_text_left_behind():
    """As in test_search_host.py: the refusals provoked here leave their text in hmpc_last_error; a successful call that needs no
    GPU ends the module with the empty text other modules start from."""
    yield
    from helpers import make_controller, _NoBackend
    from warm_start_hmpc_amd.qp_backend import jit_prebuild, load_library
    old = os.environ.get('HMPC_JIT')
    os.environ['HMPC_JIT'] = '0'
    try:
        jit_prebuild(make_controller('cart_pole_with_walls', T=10, backend=_NoBackend()).problem_data())
    finally:
        if old is None:
            del os.environ['HMPC_JIT']
        else:
            os.environ['HMPC_JIT'] = old
    assert load_library().hmpc_last_error() == b''


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    directory = tmp_path_factory.mktemp('anytime')
    return ar.build_driver(directory), directory


D = br.dims_of(SHAPE)
NFIX = D['nfix']
CAP = 96
SIZES = (0, 1, 63, 64, 65, CAP - 2, CAP - 1)


def _covers(rng, sizes=SIZES):
    return [sr.random_cover(D, n, rng) for n in sizes]


# ---- 1. the restatement, unconfigured, is its base class -----------------------------------------------------------------------------
@pytest.mark.parametrize('spec', [0, 2])
@pytest.mark.parametrize('width', [1, 8, 64])
def test_rule_zero_without_budget_is_the_base_class_on_its_own_random_covers(width, spec):
    K, rounds = len(SIZES), 4
    rows = 2 * rounds * K * width * (2 ** (spec + 1) - 1)
    a, b = sp.Search(D, K, CAP, rows, spec=spec), ar.Search(D, K, CAP, rows, spec=spec)
    covers = _covers(np.random.default_rng(width + spec))
    for s in (a, b):
        s.begin(np.zeros((K, D['nx'])), [(f, l, None, None) for f, l in covers])
    rng = np.random.default_rng(1)
    walked = 0
    for q in range(rounds):
        B = a.select(width, 0., True)
        assert b.select(width, 0., True) == B and a.P == b.P
        sr.compare_dicts(a.batch, b.batch, what=(width, spec, q))
        if a.P == 0:
            break
        rec = sr.synthetic_records(D, a.batch['fix'], rng)
        for s in (a, b):
            if B:
                s.put_records(rec)
            s.consume(0.)
        for k in range(K):
            sp.compare_tree(a.tree(k), b.tree(k), what=(width, spec, q, k))
        walked += 1
    assert walked >= 2
    sr.compare_dicts(a.results(), b.results())
    assert not (b.states() & ar.BUDGET).any()


# ---- 2. pinned to the host driver's branch_and_bound, which tests/test_bb_traces.py pins to the reference's own traces -----------------
X0 = np.array([0., 0., 1., 0.])


@pytest.fixture(scope='module')
def cart_pole_t16():
    from helpers import make_controller
    ctrl = make_controller('cart_pole_with_walls', T=16, backend='oracle', threads=8)
    return ctrl, br.dims_of(ctrl.problem_data())


@pytest.mark.parametrize('scale', [1., .5])      # (from X0 itself sixteen stages do not reach the terminal set: a search that proves infeasibility)
@pytest.mark.parametrize('rule', ['depth', 'breadth'])
@pytest.mark.parametrize('width', [1, 8])
def test_rules_solve_what_the_host_driver_solves_in_its_order(cart_pole_t16, width, rule, scale):
    from warm_start_hmpc_amd import branch_and_bound as bb
    ctrl, d = cart_pole_t16
    selection = dict(depth=bb.depth_first, breadth=bb.breadth_first)[rule]
    # the host driver: branch_and_bound(..., candidate_selection, batch_solver, frontier_width) through feedforward, its launches logged
    asked = []
    frontier = ctrl.solve_frontier

    def logged(identifiers, x0, **kw):
        asked.extend(ctrl._fix_vector(i).astype(np.int8).tobytes() for i in identifiers)
        return frontier(identifiers, x0, **kw)
    ctrl.solve_frontier = logged
    try:
        sol, leaves, solves, _ = ctrl.feedforward(X0 * scale, search_rule=selection, frontier_width=width, printing_period=None, handdown=False)
    finally:
        del ctrl.solve_frontier
    # the restatement
    ref = ar.Search(d, 1, 8192, 32768, rule=ar.RULES[rule])
    ref.begin(X0[None] * scale)
    mine = []

    def solve(x0b, fix, warm):
        mine.extend(f.tobytes() for f in fix)
        return br.as_word_records(ctrl.qp.solve_batch(x0b, fix))
    ref.run(solve, width, 0., False)
    print('%s width %d: %d solves, cost %r' % (rule, width, solves, ref.trees[0].ub))
    assert mine == asked and len(mine) == solves == ref.trees[0].solves >= 20
    res, t = ref.results(), ref.trees[0]
    assert (sol is not None) == (scale == .5)
    if sol is None:
        assert res['state'][0] == sr.DONE and np.isposinf(res['cost'][0])
    else:
        assert res['state'][0] == sr.DONE | sr.INCUMBENT and br.same_bits(np.float64(sol.objective), res['cost'][0])
        assert np.array_equal(np.rint(np.concatenate([sol.variables['ub'][s] for s in range(16)])).astype(np.int8), res['binaries'][0])
    got = [(t.fix[i].tobytes(), t.lb[i]) for i in range(len(t.lb)) if t.alive[i]]
    want = [(ctrl._fix_vector(l.identifier).astype(np.int8).tobytes(), float(l.lb)) for l in leaves]
    assert [g[0] for g in got] == [w[0] for w in want]                           # the same leaves in the same list order
    assert br.same_bits(np.array([g[1] for g in got]), np.array([w[1] for w in want]))
    b = ref.bounds(0.)
    assert b['open'][0] == 0 and b['upper'][0] == res['cost'][0]
    assert res['uncertified'][0] or b['lower'][0] >= res['cost'][0]             # proved: no leaf bounds below the incumbent


# ---- 3. the CPU form ---------------------------------------------------------------------------------------------------------------
def _case(width, rule, budget, seed, rounds=5, spec=0, row_cap=None, budgets=None, defect=None, sizes=SIZES):
    rng = np.random.default_rng(seed)
    covers = _covers(rng, sizes)
    K = len(covers)
    rows = row_cap if row_cap is not None else rounds * K * width * (2 ** (spec + 1) - 1)
    ref = ar.Search(D, K, CAP, rows, spec=spec, rule=rule, max_solves=budget, defect=defect)
    steps, refused = ar.walk(ref, D, covers, rounds, width, .03125 if width == 8 else 0., True, rng, budgets=budgets, edit=sp.scaled)
    return covers, ref, steps, refused, rows


def _budgets(width):
    return sorted(set((-1, 0, 1, width - 1, width, width + 1)))


@pytest.mark.parametrize('rule', [ar.BEST, ar.DEPTH, ar.BREADTH, ar.DIVE])
@pytest.mark.parametrize('width', [1, 8, 64])
def test_cpu_form_matches_restatement_over_rules_widths_budgets_and_sizes(driver, width, rule):
    # trees of 0, 1, 63, 64, 65, cap - 2, cap - 1 nodes (covers with runs of equal bounds and +inf bounds)
    stopped = with_inc = done = 0
    for budget in _budgets(width):
        covers, ref, steps, refused, rows = _case(width, rule, budget, 100 * width + 10 * rule + budget + 1)
        tol = .03125 if width == 8 else 0.
        out = ar.run_driver(*driver, D, len(covers), CAP, rows, covers, steps, width, tol, True, rule=rule, max_solves=budget)
        ar.compare_walk(ref, steps, out, what=(width, rule, budget))
        assert not refused and not out['refused'] and len(steps) == 5
        res = ref.results()
        if budget >= 0:
            assert (res['solves'] <= budget).all(), (budget, res['solves'])
            assert ((res['state'] & ar.BUDGET) != 0).sum() >= (3 if budget <= 1 else 0)  # (trees of 63 and more leaves outlast a budget of one)
        stopped += int(((res['state'] & ar.BUDGET) != 0).sum())
        with_inc += int((res['state'] == (ar.BUDGET | sr.INCUMBENT)).sum())
        done += int(((res['state'] & sr.DONE) != 0).sum())
        assert res['state'][0] == sr.DONE                                        # the empty tree is DONE whatever its budget
        final = steps[-1]
        assert not np.isnan(final['lower']).any() and np.isposinf(final['lower'][0])
    assert stopped > 0 and done > 0 and (width != 8 or with_inc > 0)                # (trees stopped with an incumbent too)


def test_rules_order_the_first_round_as_their_names_say(driver):
    # one tree of 65 finite, distinct bounds: best-first takes the 8 smallest bounds, depth-first nodes 64 .. 57, breadth-first 0 .. 7
    rng = np.random.default_rng(3)
    fix, lb = sr.random_cover(D, 65, rng, ties=False, infs=False)
    want = {ar.BEST: list(np.argsort(lb, kind='stable')[:8]), ar.DEPTH: list(range(64, 56, -1)), ar.BREADTH: list(range(8)), ar.DIVE: list(range(64, 56, -1))}
    for rule, nodes in want.items():
        ref = ar.Search(D, 1, CAP, 64, rule=rule)
        steps, _ = ar.walk(ref, D, [(fix, lb)], 1, 8, 0., True, np.random.default_rng(4))
        out = ar.run_driver(*driver, D, 1, CAP, 64, [(fix, lb)], steps, 8, 0., True, rule=rule)
        ar.compare_walk(ref, steps, out, what=rule)
        assert list(out['rounds'][0]['node']) == nodes, (rule, out['rounds'][0]['node'])


def test_dive_turns_best_first_once_its_tree_has_an_incumbent(driver):
    covers, ref, steps, refused, rows = _case(8, ar.DIVE, -1, 77, rounds=6)
    out = ar.run_driver(*driver, D, len(covers), CAP, rows, covers, steps, 8, .03125, True, rule=ar.DIVE)
    ar.compare_walk(ref, steps, out, what='dive')
    assert any(t.inc >= 0 for t in ref.trees) and any(t.inc < 0 and t.solves for t in ref.trees)


@pytest.mark.parametrize('spec', [1, 2])
def test_speculation_keeps_its_invariant_under_the_index_rules(driver, spec):
    # hand-down off and records that are a function of the identifier alone: picks and trees equal those at depth 0 but for row numbers
    def records(seed):
        memo = {}

        def edit(q, batch, rec):
            for b, f in enumerate(batch['fix']):
                key = f.tobytes()
                if key not in memo:
                    memo[key] = {k: np.array(rec[k][b]) for k in sr.RECORD_KEYS}
                for k in sr.RECORD_KEYS:
                    rec[k][b] = memo[key][k]
        return edit
    for rule in (ar.DEPTH, ar.BREADTH, ar.DIVE):
        walks = {}
        shared = records(rule)
        for depth in (0, spec):
            rng = np.random.default_rng(9)
            covers = [sp.cover(D, n, rng) for n in (1, 7, 20)]
            ref = ar.Search(D, 3, CAP, 4096, spec=depth, rule=rule, max_solves=11)
            steps, _ = ar.walk(ref, D, covers, 5, 3, 0., False, np.random.default_rng(5), edit=lambda q, b, r: (sp.scaled(q, b, r), shared(q, b, r)))
            out = ar.run_driver(*driver, D, 3, CAP, 4096, covers, steps, 3, 0., False, spec=depth, rule=rule, max_solves=11)
            ar.compare_walk(ref, steps, out, what=(rule, depth))
            walks[depth] = (ref, steps)
        (a, sa), (b, sb) = walks[0], walks[spec]
        assert b.count['served'] > 0
        for q, (x, y) in enumerate(zip(sa, sb)):
            assert x['P'] == y['P'], (rule, q)
            assert np.array_equal(x['state'], y['state']) and br.same_bits(x['lower'], y['lower']) and np.array_equal(x['open'], y['open'])
        for k in range(3):
            sp.compare_modulo_rows(a.tree(k), b.tree(k), a.pool, b.pool, what=(rule, spec, k))


def _small_and_large(row_cap):
    """Trees of 1 (a root, whose record branches), 65 and 64 leaves under a budget of 8 at width 8: round 0 spends the budget of
    the large trees, round 1 picks the small tree's two children and finds the large ones out of budget."""
    rng = np.random.default_rng(21)
    covers = [(np.full((1, NFIX), -1, np.int8), np.array([.125]))] + _covers(rng, (65, 64))

    def edit(q, batch, rec):
        sp.scaled(q, batch, rec)
        if q == 0:
            rec['status'][0], rec['obj'][0], rec['iters'][0] = 0, .25, br.POLISHED_BIT | 3
    ref = ar.Search(D, 3, CAP, row_cap, rule=ar.BEST, max_solves=8)
    steps, refused = ar.walk(ref, D, covers, 2, 8, 0., True, rng, edit=edit)
    return covers, ref, steps, refused


def test_a_round_refused_for_row_cap_changes_nothing_under_an_exhausted_budget(driver):
    covers, big, steps, refused = _small_and_large(64)
    assert not refused and (steps[0]['B'], steps[1]['B']) == (17, 2) and list(steps[1]['state'] & ~sr.INCUMBENT) == [0, ar.BUDGET, ar.BUDGET]
    # a pool one row short of round 1 refuses it -- and the words of the two trees that are out of budget stay 0, as every other
    covers, ref, short, refused = _small_and_large(18)
    assert refused and len(short) == 1 and list(ref.states()) == [0, 0, 0]
    out = ar.run_driver(*driver, D, 3, CAP, 18, covers, steps, 8, 0., True, rule=ar.BEST, max_solves=8)
    assert out['refused']
    ar.compare_walk(ref, short, out, what='refused')
    # ... and in a pool that holds it exactly the same round stops them
    covers, ref, full, refused = _small_and_large(19)
    out = ar.run_driver(*driver, D, 3, CAP, 19, covers, full, 8, 0., True, rule=ar.BEST, max_solves=8)
    ar.compare_walk(ref, full, out, what='fits')
    assert not refused and not out['refused'] and list(out['rounds'][1]['state'] & ~sr.INCUMBENT) == [0, ar.BUDGET, ar.BUDGET]


def test_set_budget_reopens_stopped_trees_and_a_spent_budget_stops_them_again(driver):
    budgets = {0: 3, 2: 3, 3: 12, 5: -1}                                         # 3: stop; 3 again: stop again at once; 12: on; none: to the end
    covers, ref, steps, refused, rows = _case(8, ar.DIVE, -1, 31, rounds=8, budgets=budgets)
    out = ar.run_driver(*driver, D, len(covers), CAP, rows, covers, steps, 8, .03125, True, rule=ar.DIVE, max_solves=-1)
    ar.compare_walk(ref, steps, out, what='reopen')
    stopped = [(s['state'] & ar.BUDGET) != 0 for s in steps]
    assert stopped[1].any() and np.array_equal(stopped[1], stopped[2]) and steps[2]['P'] == 0      # the same budget again: no pick, the same words
    assert steps[3]['P'] > 0 and not (steps[3]['state'][stopped[2]] & ar.BUDGET).any()             # a larger one: they run again
    assert not stopped[-1].any() and steps[5]['P'] > 0
    # DONE, FAILED and OVERFLOW trees are not reopened
    for q in (3, 5):
        before, after = steps[q - 1]['state'], steps[q]['state']
        keep = (before & (sr.DONE | sr.FAILED | sr.OVERFLOW)) != 0
        assert np.array_equal(before[keep], after[keep])


# ---- 4. planted defects --------------------------------------------------------------------------------------------------------------
def _defect_case(defect, planted):
    """(covers, restatement after its walk, steps, rows, rule, budget) on which the defect shows."""
    if defect == 'lower_forgets_unc_lb':
        # two leaves bounded .125 and .5; the first is solved into an uncertified proof of infeasibility: the tree has proved .125, not .5
        fix = np.full((2, NFIX), -1, np.int8)
        fix[:, 0] = [0, 1]
        covers = [(fix, np.array([.125, .5]))]

        def edit(q, batch, rec):
            if q == 0:
                rec['status'][0], rec['obj'][0], rec['iters'][0] = 1, np.inf, br.UNCERTIFIED_BIT | br.WEAK_BIT | 3
        ref = ar.Search(D, 1, CAP, 8, rule=ar.BEST, max_solves=1, defect=planted)
        steps, _ = ar.walk(ref, D, covers, 2, 1, 0., True, np.random.default_rng(2), edit=edit)
        return covers, ref, steps, 8, 1, ar.BEST, 1
    rule, budget = (ar.DEPTH, -1) if defect == 'depth_by_bound' else (ar.BEST, 11)
    covers, ref, steps, _, rows = _case(8, rule, budget, 55, rounds=4, defect=planted)
    return covers, ref, steps, rows, 8, rule, budget


@pytest.mark.parametrize('defect', sorted(ar.DEFECTS))
def test_planted_defects_fail_the_comparison(driver, defect):
    covers, ref, steps, rows, width, rule, budget = _defect_case(defect, None)
    tol = .03125 if width == 8 else 0.
    args = (D, len(covers), CAP, rows, covers, steps, width, tol, True)
    good = ar.run_driver(*driver, *args, rule=rule, max_solves=budget)
    ar.compare_walk(ref, steps, good, what=defect)
    if defect == 'lower_forgets_unc_lb':
        assert list(steps[-1]['lower']) == [.125] and steps[-1]['state'][0] == ar.BUDGET and ref.trees[0].unc_lb == .125
    with pytest.raises(AssertionError):                                          # (a walk that stages another number of rows ends the driver: an assertion too)
        bad = ar.run_driver(*driver, *args, rule=rule, max_solves=budget, defect=ar.DEFECTS[defect])
        ar.compare_walk(ref, steps, bad, what=defect)
    # ... and the restatement with the same defect planted walks the defective walk
    covers, twin, steps2, rows, width, rule, budget = _defect_case(defect, defect)
    bad = ar.run_driver(*driver, D, len(covers), CAP, rows, covers, steps2, width, tol, True, rule=rule, max_solves=budget, defect=ar.DEFECTS[defect])
    ar.compare_walk(twin, steps2, bad, what=(defect, 'twin'))
    if defect == 'lower_forgets_unc_lb':
        assert list(bad['rounds'][-1]['lower']) == [.5]


# ---- 5. header and binding -----------------------------------------------------------------------------------------------------------
def test_header_and_binding_name_the_same_symbols_rules_and_stop_state():
    from warm_start_hmpc_amd import qp_backend
    header = open(os.path.join(ROOT, 'include', 'hmpc_search_anytime.h')).read()
    declared = re.findall(r'^int\s+(hmpc_[a-z_]+)\s*\(', header, re.M)
    assert tuple(declared) == qp_backend.EXPORTED_SEARCH_ANYTIME_SYMBOLS and len(declared) == 3
    assert not set(declared) & set(qp_backend.EXPORTED_SYMBOLS) and not set(declared) & set(qp_backend.EXPORTED_SEARCH_SYMBOLS)
    lib = qp_backend.load_library()
    for name in declared:
        assert getattr(lib, name) is not None
    rules = dict((name, int(v)) for name, v in re.findall(r'#define HMPC_RULE_([A-Z_]+)\s+(\d+)\b', header))
    assert rules == dict(BEST_FIRST=0, DEPTH_FIRST=1, BREADTH_FIRST=2, DIVE_THEN_BEST=3)
    assert qp_backend.SEARCH_RULES == dict(best=ar.BEST, depth=ar.DEPTH, breadth=ar.BREADTH, dive=ar.DIVE) == ar.RULES
    stops = dict((name.lower(), int(v, 16)) for name, v in re.findall(r'#define HMPC_SEARCH_([A-Z_]+)\s+(0x[0-9a-fA-F]+)\b', header))
    assert stops == qp_backend.SEARCH_STOP_STATES == dict(budget=ar.BUDGET)
    assert not ar.BUDGET & sum(qp_backend.SEARCH_STATES.values())                # a bit of its own
    # the header of the first search entries and the kernels' key are as they were
    assert 'anytime' not in open(os.path.join(ROOT, 'include', 'hmpc_search.h')).read()
    assert qp_backend.SEARCH_STATES == dict(done=0x1, incumbent=0x2, failed=0x4, overflow=0x8) and len(qp_backend.EXPORTED_SEARCH_SYMBOLS) == 19


# ---- 6. refusals without a GPU -------------------------------------------------------------------------------------------------------
def test_the_new_entries_refuse_bad_arguments_without_touching_the_gpu():
    from warm_start_hmpc_amd.qp_backend import load_library
    lib = load_library()
    for rule in (-1, 4):                                                        # the range comes first: no search is needed to refuse it
        assert lib.hmpc_search_set_rule(None, rule) == -1 and b'0 .. 3' in lib.hmpc_last_error()
    for rule in (0, 3):
        assert lib.hmpc_search_set_rule(None, rule) == -1 and b'null' in lib.hmpc_last_error()
    for m in (-1, 0, 5):
        assert lib.hmpc_search_set_budget(None, m, None) == -1 and b'null' in lib.hmpc_last_error()
    out = np.full(3, -7.)
    assert lib.hmpc_search_bounds(None, 0., out.ctypes.data, None, None, None) == -1 and b'null' in lib.hmpc_last_error()
    assert (out == -7.).all()
