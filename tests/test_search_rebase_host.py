"""hmpc_search_rebase (include/hmpc_search.h) without a GPU: the per-item functions of csrc/hmpc_search.h -- what the lanes of the
retain, stage, rebase-rows and adopt kernels run -- walked serially over K trees (tests/host/rebase_driver.cpp) under AddressSanitizer
and UBSan with contraction off, held to the numpy restatement of tests/rebase_reference.py (integers exactly, floats bit for bit)
through begin -> synthetic rounds -> two re-bases in a row -> rounds -> an advance; trees in every state and leaves of every kind a
re-base tells apart; the pool exactly full and one row short; three planted defects, each of which the comparison must catch; the
entry's argument checks."""
import numpy as np
import pytest

import branch_reference as br
import rebase_reference as rr
import search_reference as sr
from test_search_advance_host import SIZES, STATES, CASES, dims

PLAN = ['finish', 'rebase', 'rebase', 'finish', 'advance']                       # the second re-base starts from the first one's dual_obj
RUNNING = ['rounds:1', 'rebase', 'rounds:2', 'rebase0', 'rebase', 'finish', 'advance']


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    directory = tmp_path_factory.mktemp('rebase')
    return rr.build_driver(directory), directory


def both(driver, d, specs, node_cap, row_cap, with_rows, seed, plan, planted=None, roots=False):
    ref, x0s, (covers, rows), ops = rr.walk(d, specs, node_cap, row_cap, with_rows, seed, plan, roots=roots)
    got, row0 = rr.run_driver(*driver, d, len(specs), node_cap, row_cap, x0s, covers, rows, ops, defect=planted)
    return ref, [op for op in ops if op[0] != 'round'], got, row0


def compare(ref, ops, got, row0, what=''):
    assert len(ops) == len(got)
    for q, (op, g) in enumerate(zip(ops, got)):
        want, trees = op[2], op[3]
        if want is sr.TooBig:
            assert g['rc'] == -3, (what, q)
        else:
            assert g['rc'] == 0 and g['B'] == want['B'], (what, q, g['rc'])
            keys = rr.REBASE_KEYS if op[0] == 'rebase' else ('owner', 'src', 'lb', 'cover', 'reopened')
            sr.compare_dicts({k: want[k] for k in keys}, g, what=(what, op[0], q))
            if op[0] == 'advance':
                assert br.same_bits(want['x0_next'], g['x0'])
        for k in range(ref.K):
            sr.compare_tree(trees[k], g['trees'][k], what=(what, op[0], q, 'tree', k))
    assert row0 == ref.row0


def rebases(ops):
    return [op[2] for op in ops if op[0] == 'rebase']


@pytest.mark.parametrize('name', ['random_mld_t5', 'cart_pole_t16'])
@pytest.mark.parametrize('case', ['sizes', 'states', 'one'])
@pytest.mark.parametrize('with_rows', [True, False])
def test_driver_walks_the_restatement_through_rebases_and_an_advance(driver, name, case, with_rows):
    # trees of 1, 63, 64, 65 and 129 nodes with dead nodes in between; DONE | INCUMBENT, DONE without incumbent, FAILED, OVERFLOW;
    # covers without rows (row < 0: the row of zeros, reopened) and with rows of which some are weak; +inf leaves whose proof
    # survives and does not; the -inf root a FAILED tree has become, re-based again; then rounds and an advance on what is left
    d = dims(name)
    specs, node_cap = CASES[case]
    ref, ops, got, row0 = both(driver, d, specs, node_cap, 4096, with_rows, len(name) + 7 * with_rows, PLAN)
    compare(ref, ops, got, row0, what=(name, case, with_rows))
    first, second = rebases(ops)
    if case == 'sizes':
        assert first['B'] > 64 and [len(t['lb']) for t in ops[0][3]] == list(first['cover'])
    if case == 'states':
        assert list(first['cover'][2:4]) == [0, 0] and first['cover'][0] > 0 and first['cover'][4] > 0
        assert list(second['cover'][2:4]) == [1, 1] and np.all(np.isneginf(second['lb'][second['owner'] == 2]))   # the -inf root, re-based
        assert list(second['reopened'][2:4]) == [1, 1]
    if with_rows:
        inf = np.isposinf(first['lb'])
        assert (np.isposinf(first['lb_out'][inf])).any() and (first['lb_out'][inf] == 0.).any()   # a proof that survives, one that does not
        assert (first['src'] < 4096).all() and first['reopened'].sum() == (inf & (first['lb_out'] == 0.)).sum()
    else:
        assert (first['src'] == 4096).any() and (first['src'] < 4096).any() and first['reopened'].sum() >= (first['src'] == 4096).sum()
    assert case == 'states' or np.array_equal(second['src'], np.arange(second['B']))   # the pool was compacted: leaf b carries row b
    assert not br.same_bits(first['dual_obj'], second['dual_obj'][:first['B']]) or first['B'] == 0


@pytest.mark.parametrize('name', ['random_mld_t5', 'cart_pole_t16'])
def test_running_trees_take_part_and_weak_rows_reopen(driver, name):
    d = dims(name)
    ref, ops, got, row0 = both(driver, d, STATES, 160, 4096, True, 4, RUNNING)
    compare(ref, ops, got, row0, what=(name, 'running'))
    first, same, third = rebases(ops)
    assert first['cover'][4] > 0 and list(first['cover'][2:4]) == [0, 0]
    before = rr.walk(d, STATES, 160, 4096, True, 4, ['rounds:1'])[0]
    assert before.trees[4].state == 0 and before.trees[4].inc >= 0 and before.trees[2].state == sr.FAILED and before.trees[3].state == sr.OVERFLOW
    # a weak row reopens its +inf leaf, whatever the state
    pool = before.pool['dual_obj']
    weak = np.isneginf(pool[np.minimum(first['src'], 4095)]) & (first['src'] < 4096)
    assert weak.any() and np.all(first['dual_obj'][weak] == 0.) and np.all(first['lb_out'][weak] == 0.)
    # delta = 0: the rows' dual objectives only lose what is below zero, and no bound with a sound row moves
    sound = same['dual_obj'] > 0.
    assert sound.any() and np.all(same['lb_out'][sound & np.isfinite(same['lb'])] == same['dual_obj'][sound & np.isfinite(same['lb'])])


@pytest.mark.parametrize('name', ['random_mld_t5', 'cart_pole_t16'])
def test_roots_are_rebased_as_the_shift_moves_them(driver, name):
    d = dims(name)
    ref, ops, got, row0 = both(driver, d, SIZES, 420, 4096, False, 2, ['rebase', 'rounds:2', 'rebase'], roots=True)
    compare(ref, ops, got, row0, what=(name, 'roots'))
    first = rebases(ops)[0]
    assert first['B'] == 5 and np.all(np.isneginf(first['lb'])) and np.all(first['lb_out'] == 0.) and list(first['reopened']) == [1] * 5


def test_pool_exactly_full_and_one_row_short(driver):
    d = dims('random_mld_t5')
    plan = ['finish', 'rebase', 'rounds:1']
    B = rebases(both(driver, d, SIZES, 420, 4096, False, 3, plan)[1])[0]['B']
    assert B > 64
    ref, ops, got, row0 = both(driver, d, SIZES, 420, B, False, 3, ['finish', 'rebase'])          # kept total == row_cap
    compare(ref, ops, got, row0, what='full')
    assert rebases(ops)[0]['B'] == B == row0 and (rebases(ops)[0]['src'] == B).any()
    # one row short: refused, and the trees are those the step ended with; the walk goes on from them
    ref, ops, got, row0 = both(driver, d, SIZES, 420, B - 1, False, 3, ['finish', 'rebase', 'advance'])
    assert ops[0][2] is sr.TooBig and got[0]['rc'] == -3
    ended = rr.walk(d, SIZES, 420, B - 1, False, 3, ['finish'])[0]
    for k in range(5):
        sr.compare_tree(ended.tree(k), got[0]['trees'][k], what=('refused', k))
    compare(ref, ops, got, row0, what='short')


@pytest.mark.parametrize('defect', ['bound_from_lb', 'stale_dual_obj', 'failed_keeps_leaves'])
def test_planted_defects_fail_the_comparison(driver, defect):
    d = dims('random_mld_t5')
    args = (d, STATES, 160, 4096, True, 4, ['finish', 'rebase', 'rebase'])
    compare(*both(driver, *args), what='sound')
    with pytest.raises(AssertionError):
        compare(*both(driver, *args, planted=defect), what=defect)


@pytest.fixture(scope='module')
def oracle_trees():
    """The cart-pole with walls at T = 20 from rebase_reference.states(), searched cold by the restatement on the CPU oracle's records."""
    from helpers import make_controller, load_fixture
    ctrl = make_controller('cart_pole_with_walls', T=20, backend='oracle')
    d = br.dims_of(ctrl.problem_data())
    solve = lambda x0, fix, warm: br.as_word_records(ctrl.qp.solve_batch(x0, fix))

    def cold(x0s):
        ref = rr.Search(d, len(x0s), 4096, 16384)
        ref.begin(x0s)
        ref.run(solve, 8, rr.SEARCH_TOL, False)
        return ref
    return ctrl, solve, cold, load_fixture('cart_pole_with_walls')['x_max']


@pytest.mark.parametrize('scale', [.003, 0.])
def test_oracle_trees_rebase_to_bounds_and_end_where_cold_searches_end(oracle_trees, scale):
    # the CPU form of tests/test_gpu_search_rebase.py (b) and (c): the restatement on the oracle's records.  At delta = 0 it is the
    # confirmation the one-round condition of (c) asks for: on these trees no leaf is reopened and every tree finishes in one round
    ctrl, solve, cold, x_max = oracle_trees
    x0s = rr.states()
    xn = rr.measured(x0s, x_max, scale)
    ref = cold(x0s)
    first = ref.results()
    assert not np.any(first['state'] & (sr.FAILED | sr.OVERFLOW)) and np.isfinite(first['cost']).any()
    out = ref.rebase(xn)
    assert np.array_equal(out['cover'], first['leaves']) and out['B'] > 100
    leaves = ref.leaves()
    rr.check_bounds(leaves['lb'], solve(xn[leaves['owner']], leaves['fix'], None), rr.gap_allowance(ctrl), what='oracle, scale %g' % scale)
    ref.run(solve, 8, rr.SEARCH_TOL, False, max_rounds=1)
    mid = ref.results()
    rest = ref.run(solve, 8, rr.SEARCH_TOL, False)
    last, want = ref.results(), cold(xn).results()
    print('oracle, scale %g: cold solves %s, reopened %s, re-based solves %s (round one %s, then %d rounds)' % (scale, first['solves'], out['reopened'], last['solves'], mid['solves'], rest[0]))
    assert np.all(np.isclose(last['cost'], want['cost'], rtol=1e-5) | (np.isinf(last['cost']) & np.isinf(want['cost'])))
    assert np.array_equal(last['binaries'], want['binaries'])
    if scale == 0.:
        few = out['reopened'] < 8
        assert few.any() and np.array_equal(last['solves'][few], mid['solves'][few])


def test_header_binding_and_null_arguments():
    from warm_start_hmpc_amd import qp_backend
    lib = qp_backend.load_library()
    assert 'hmpc_search_rebase' in qp_backend.EXPORTED_SEARCH_SYMBOLS and lib.hmpc_search_rebase is not None
    cover, x0 = np.full(3, -7, np.int32), np.zeros(12)
    assert lib.hmpc_search_rebase(None, x0.ctypes.data, cover.ctypes.data, None, None) == -1 and b'null argument' in lib.hmpc_last_error()
    assert np.all(cover == -7)
    assert lib.hmpc_search_destroy(None) == 0 and lib.hmpc_last_error() == b''   # (other modules start from the empty text)
    from warm_start_hmpc_amd.search import DeviceSearch
    import inspect
    assert inspect.signature(DeviceSearch.closed_loop).parameters['presolve'].default is False
    assert inspect.signature(DeviceSearch.closed_loop).parameters['resident'].default is False
    assert inspect.signature(DeviceSearch.rebase).parameters['stats'].default is True
