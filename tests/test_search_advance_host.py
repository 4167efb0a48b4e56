"""hmpc_search_advance (include/hmpc_search.h) without a GPU: the per-tree functions of csrc/hmpc_search.h -- what the lanes of the
retain, stage and adopt kernels run -- walked serially over K trees (tests/host/advance_driver.cpp) under AddressSanitizer and UBSan,
held to the numpy restatement of tests/advance_reference.py (integers exactly, floats bit for bit) through begin -> synthetic rounds ->
advance, twice in a row; three planted defects, each of which the comparison must catch; the refusals; the entry's argument checks."""

import numpy as np
import pytest

import advance_reference as ar
import branch_reference as br
import search_reference as sr


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    directory = tmp_path_factory.mktemp('advance')
    return ar.build_driver(directory), directory


def _dims(name):
    """The sizes of the GPU half's problems (tests/test_gpu_branch.py: _backend), from the same builders, without a backend."""
    from helpers import make_controller, random_mld, _NoBackend
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    if name == 'random_mld_t5':
        mld, objective, _ = random_mld(nx=6, nuc=2, nub=3, seed=3)
        ctrl = HybridModelPredictiveController(mld, 5, objective, None, backend=_NoBackend())
    else:
        ctrl = make_controller('cart_pole_with_walls', T=16, backend=_NoBackend())
    return br.dims_of(ctrl.problem_data())


_DIMS = {}


def dims(name):
    if name not in _DIMS:
        _DIMS[name] = _dims(name)
    return _DIMS[name]


SIZES = [dict(kind='inc', m=1, c=0), dict(kind='inc', m=43, c=10), dict(kind='inc', m=44, c=10), dict(kind='inc', m=45, c=10), dict(kind='inc', m=89, c=20)]
STATES = [dict(kind='none', m=5), dict(kind='disagree', m=12, c=3), dict(kind='failed', m=6), dict(kind='overflow'), dict(kind='inc', m=20, c=6)]
CASES = {'sizes': (SIZES, 420), 'states': (STATES, 160), 'one': (SIZES[4:], 420)}


def walk(d, specs, node_cap, row_cap, with_rows, seed, n_steps=2, defect=None, drop=(), x0_given=False):
    """The restatement's walk, recorded for the driver: (ref, x0s, covers, steps, staged per step)."""
    rng = np.random.default_rng(seed)
    K = len(specs)
    covers, u0b = ar.make_covers(d, specs, rng, node_cap)
    x0s = rng.uniform(-1., 1., (K, d['nx']))
    ref = ar.Search(d, K, node_cap, row_cap, defect=defect)
    ref.begin(x0s, [(f, l, np.zeros((len(l), d['n_dual'])) if with_rows else None, np.zeros(len(l)) if with_rows else None) for f, l in covers])
    steps, staged = [], []
    for step in range(n_steps):
        rounds = ar.run_step(ref, d, specs, u0b, rng)
        kept = {}
        inner = ar.synthetic_shift(d, rng, drop=drop if step == 0 else ())

        def shift(st, kept=kept, inner=inner):
            kept.update(inner(st))
            return kept
        e0 = rng.uniform(-.1, .1, (K, d['nx'])) if step == 0 else None
        xn = rng.uniform(-1., 1., (K, d['nx'])) if x0_given and step == 0 else None
        staged.append(ref.advance(shift, e0, xn))
        steps.append((rounds, dict(e0=e0, x0_next=xn, **kept)))
    return ref, x0s, covers, steps, staged


def both(driver, d, specs, node_cap, row_cap, with_rows, seed, planted=None, **kw):
    ref, x0s, covers, steps, staged = walk(d, specs, node_cap, row_cap, with_rows, seed, **kw)
    advances, trees, row0 = ar.run_driver(*driver, d, len(specs), node_cap, row_cap, x0s, covers, with_rows, steps, defect=planted)
    return ref, staged, advances, trees, row0


def compare(ref, staged, advances, trees, row0, what=''):
    assert len(advances) == len(staged)
    for q, (a, b) in enumerate(zip(staged, advances)):
        assert b['rc'] == 0 and b['B'] == a['B'], (what, q)
        sr.compare_dicts({k: a[k] for k in ar.STAGED_KEYS}, b, what=(what, 'advance', q))
    for k in range(ref.K):
        sr.compare_tree(ref.tree(k), trees[k], what=(what, 'tree', k))
    assert row0 == ref.row0


@pytest.mark.parametrize('name', ['random_mld_t5', 'cart_pole_t16'])
@pytest.mark.parametrize('case', ['sizes', 'states', 'one'])
@pytest.mark.parametrize('with_rows', [True, False])
def test_driver_walks_the_restatement_through_two_advances(driver, name, case, with_rows):
    # trees of 1, 63, 64, 65 and 129 nodes with dead nodes in between (a cover of m leaves of which c branch once the incumbent is
    # there), children that share their parent's row, a tree without incumbent, one whose every leaf disagrees, a FAILED and an
    # OVERFLOW one; covers without rows: every unsolved leaf has row < 0 and shifts from the row of zeros; the second advance reads
    # what the first one wrote
    d = dims(name)
    specs, node_cap = CASES[case]
    ref, staged, advances, trees, row0 = both(driver, d, specs, node_cap, 4096, with_rows, seed=len(name) + 7 * with_rows, x0_given=case == 'one')
    compare(ref, staged, advances, trees, row0, what=(name, case, with_rows))
    first = staged[0]
    if case == 'sizes':
        assert all(c > 0 for c in first['cover']) and first['B'] > 64
    if case == 'states':
        assert list(first['cover'][:4]) == [0, 0, 0, 0] and first['cover'][4] > 0
        assert np.all(first['u0'][[0, 2, 3]] == 0.) and np.any(first['u0'][1] != 0.)
    if not with_rows:
        assert (first['src'] == 4096).any() and (first['src'] < 4096).any() and first['reopened'].sum() >= (first['src'] == 4096).sum()
    elif case != 'states':
        assert (np.bincount(first['src']) > 1).any()                             # siblings that share their parent's row
    assert (staged[1]['B'] > 0 or case == 'states') and ref.row0 == staged[1]['B']   # (an advance that keeps nothing is one too)


def test_the_first_step_ends_with_the_trees_the_issue_lists(driver):
    d = dims('random_mld_t5')
    rng = np.random.default_rng(1)
    covers, u0b = ar.make_covers(d, SIZES + STATES, rng, 160)
    ref = ar.Search(d, 10, 160, 4096)
    ref.begin(np.zeros((10, d['nx'])), [(f, l, None, None) for f, l in covers])
    ar.run_step(ref, d, SIZES + STATES, u0b, rng)
    assert [len(t.lb) for t in ref.trees[:5]] == [1, 63, 64, 65, 129]
    assert all(not all(t.alive) for t in ref.trees[1:5])                         # dead nodes in between
    assert [t.state for t in ref.trees] == [ar.ADVANCES] * 5 + [sr.DONE, ar.ADVANCES, sr.FAILED, sr.OVERFLOW, ar.ADVANCES]
    assert ref.retained(ref.trees[6]) == [] and all(ref.retained(ref.trees[k]) for k in (0, 1, 2, 3, 4, 9))


def test_pool_exactly_full_and_one_row_short(driver):
    d = dims('random_mld_t5')
    specs, node_cap = SIZES, 420
    probe = walk(d, specs, node_cap, 4096, False, seed=3, n_steps=1)[4][0]
    B = probe['B']
    ref, staged, advances, trees, row0 = both(driver, d, specs, node_cap, B, False, seed=3, n_steps=1)   # kept total == row_cap
    compare(ref, staged, advances, trees, row0, what='full')
    assert staged[0]['B'] == B == row0 and (staged[0]['src'] == B).any()
    # one row short: refused, and the trees are those the step ended with
    rng = np.random.default_rng(3)
    covers, u0b = ar.make_covers(d, specs, rng, node_cap)
    x0s = rng.uniform(-1., 1., (5, d['nx']))
    ref = ar.Search(d, 5, node_cap, B - 1)
    ref.begin(x0s, [(f, l, None, None) for f, l in covers])
    rounds = ar.run_step(ref, d, specs, u0b, rng)
    before = [ref.tree(k) for k in range(5)]
    with pytest.raises(sr.TooBig):
        ref.advance(ar.synthetic_shift(d, rng))
    nothing = dict(fix_out=np.zeros((0, d['nfix']), np.int8), lb_out=np.zeros(0), flags=np.zeros(0, np.uint8))
    advances, trees, row0 = ar.run_driver(*driver, d, 5, node_cap, B - 1, x0s, covers, False, [(rounds, nothing)])
    assert [a['rc'] for a in advances] == [-3] and row0 == ref.row0
    for k in range(5):
        sr.compare_tree(before[k], trees[k], what=('refused', k))
        sr.compare_tree(ref.tree(k), trees[k], what=('restatement refused', k))


def test_a_running_tree_is_refused(driver):
    d = dims('random_mld_t5')
    rng = np.random.default_rng(4)
    covers, u0b = ar.make_covers(d, STATES, rng, 160)
    x0s = np.zeros((5, d['nx']))
    ref = ar.Search(d, 5, 160, 4096)
    ref.begin(x0s, [(f, l, None, None) for f, l in covers])
    assert ref.select(1, 0., True) > 0
    rec = ar.records_for(ref, d, STATES, u0b, rng)
    ref.put_records(rec)
    ref.consume(0.)                                                              # one round: the last tree has its incumbent and candidates left
    assert ref.trees[4].state == 0 and ref.trees[4].inc >= 0
    before = [ref.tree(k) for k in range(5)]
    with pytest.raises(ar.Invalid):
        ref.advance(ar.synthetic_shift(d, rng))
    nothing = dict(fix_out=np.zeros((0, d['nfix']), np.int8), lb_out=np.zeros(0), flags=np.zeros(0, np.uint8))
    advances, trees, _ = ar.run_driver(*driver, d, 5, 160, 4096, x0s, covers, False, [([(1, rec)], nothing)])
    assert [a['rc'] for a in advances] == [-1]
    for k in range(5):
        sr.compare_tree(before[k], trees[k], what=('running', k))


TINY = [dict(kind='inc', m=2, c=1)]      # a complete leaf and one that branches: nodes 0 (incumbent), 1 (dead), 2, 3 (children, wrow = their parent's row)


@pytest.mark.parametrize('defect', ['no_rint', 'keeps_wrow', 'silent_drop'])
def test_planted_defects_fail_the_comparison(driver, defect):
    d = dims('random_mld_t5')
    # seeds whose trees show the defect: an incumbent binary of 0.9999999 that a kept leaf fixes at 1; a vertex record (wrow >= 0)
    # in a slot the cover takes; a dropped leaf
    seed = {'no_rint': 0, 'keeps_wrow': 1, 'silent_drop': 0}[defect]
    specs, cap = (TINY, 8) if defect == 'keeps_wrow' else (SIZES, 420)
    kw = dict(n_steps=1, drop=(1,) if defect == 'silent_drop' else ())
    while True:                                                                  # (the first seed at which the defect is visible in the restatement)
        good = walk(d, specs, cap, 4096, True, seed, **kw)
        twin = walk(d, specs, cap, 4096, True, seed, defect=defect, **kw)
        try:
            for k in range(len(specs)):
                sr.compare_tree(good[0].tree(k), twin[0].tree(k))
        except AssertionError:
            break
        seed += 1
        assert seed < 40, 'no seed shows the defect'
    ref, staged, advances, trees, row0 = both(driver, d, specs, cap, 4096, True, seed, **kw)
    compare(ref, staged, advances, trees, row0, what='sound')
    if defect == 'silent_drop':
        assert sr.FAILED in [t['state'] for t in trees]
    with pytest.raises(AssertionError):
        compare(*both(driver, d, specs, cap, 4096, True, seed, planted=defect, **kw), what=defect)
    # ... and the restatement with the same defect planted walks the defective walk
    compare(*both(driver, d, specs, cap, 4096, True, seed, planted=defect, defect=defect, **kw), what=(defect, 'twin'))


def test_header_binding_and_null_search():
    from warm_start_hmpc_amd import qp_backend
    lib = qp_backend.load_library()
    assert 'hmpc_search_advance' in qp_backend.EXPORTED_SEARCH_SYMBOLS and lib.hmpc_search_advance is not None
    cover = np.full(3, -7, np.int32)
    assert lib.hmpc_search_advance(None, None, None, cover.ctypes.data, None, None) == -1 and b'null search' in lib.hmpc_last_error()
    assert np.all(cover == -7)
    assert lib.hmpc_search_destroy(None) == 0 and lib.hmpc_last_error() == b''   # (other modules start from the empty text)
    from warm_start_hmpc_amd.search import DeviceSearch
    import inspect
    assert inspect.signature(DeviceSearch.closed_loop).parameters['resident'].default is False
    assert inspect.signature(DeviceSearch.advance).parameters['stats'].default is True
