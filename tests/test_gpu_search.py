"""The device-resident search on the device (csrc/hmpc_search.hip behind include/hmpc_search.h), held to the numpy restatement of
tests/search_reference.py -- integers exactly, floats bit for bit: synthetic rounds through begin(cover) / select / put_records /
consume on the edges of the kernels; whole searches of the cart-pole with walls (T = 20) against the restatement driven by the
same handle's solve_batch; three closed-loop steps against BatchedMPC.closed_loop on the same backend."""
import ctypes

import numpy as np
import pytest

import branch_reference as br
import search_reference as sr
from test_gpu_branch import _backend

pytestmark = pytest.mark.gpu
SCAN_CHUNK = 1024          # SEARCH_SCAN_CHUNK of csrc/hmpc_search.hip: trees per pass of the offsets kernel
X0 = np.array([0., 0., 1., 0.])                                                # (tests/test_fleet.py)
INFEASIBLE = np.array([0., 0., 5., 0.])                                       # (test_fleet_stops_a_loop_whose_miqp_is_infeasible_and_resets)


def _search(name, K, node_cap, row_cap):
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, qp, d = _backend(name)
    return DeviceSearch(ctrl, K, node_cap=node_cap, row_cap=row_cap), d


def _cover_arrays(covers):
    from warm_start_hmpc_amd.batched import NodeArrays
    return [NodeArrays(np.ascontiguousarray(f), np.ascontiguousarray(l), dual, dobj, np.ones(len(l), bool)) for f, l, dual, dobj in covers]


def _same_state(ds, ref, what, trees=None):
    sr.compare_dicts(ref.results(), ds.results(), what=(what, 'results'))
    sr.compare_dicts(ref.leaves(), ds.leaves_flat(), what=(what, 'leaves'))
    for k in (range(ds.K) if trees is None else trees):
        sr.compare_tree(ref.tree(k), ds.tree(k), what=(what, 'tree', k))


def _round(ds, ref, d, width, tol, handdown, rng, what, plan=None):
    """One synthetic round on both; returns its size."""
    B = ref.select(width, tol, handdown)
    assert ds.select(width, tol, handdown) == B, what
    if B == 0:
        return 0
    got = ds.batch()
    sr.compare_dicts(ref.batch, got, what=(what, 'batch'))
    rec = sr.synthetic_records(d, ref.batch['fix'], rng, plan=plan(ref.batch) if plan else None)
    ref.put_records(rec)
    ds.put_records(rec)
    ref.consume(tol)
    ds.consume(tol)
    return B


SIZES = lambda cap: (1, 63, 64, 65, cap - 2, cap - 1, 0)


@pytest.mark.parametrize('name,K,width,tol', [('random_mld_t5', 1, 1, 0.), ('random_mld_t5', 5, 8, .5), ('cart_pole_t16', 7, 64, 0.),
                                              ('cart_pole_t20', 7, 8, .5), ('random_mld_t5', SCAN_CHUNK + 1, 8, 0.),
                                              ('cart_pole_t16', 3, 1, .5)])
def test_synthetic_rounds_on_the_edges_of_the_kernels(name, K, width, tol):
    # trees of 1, 63, 64, 65, node_cap - 2, node_cap - 1 leaves (one wave of nodes, one more, a slab that takes one branch, one
    # that takes none) and, in between, trees without a leaf or with +inf bounds only: no candidates; K = 1025: one tree past the
    # 1024 the offsets kernel scans per pass; width 64 on a tree of one leaf: wider than the candidates; bounds in runs of equal
    # values (first wins) and +inf (never picked)
    cap = 96
    rng = np.random.default_rng(K * 100 + width)
    ds, d = _search(name, K, cap, 3 * K * min(width, cap) + K * cap)
    sizes = [SIZES(cap)[(k + (3 if K == 1 else 1)) % 7] for k in range(K)]      # (tree K - 1 of 1025 has 65 leaves)
    covers = []
    for k, n in enumerate(sizes):
        f, l = sr.random_cover(d, n, rng)
        if k % 7 == 2 and k != K - 1:
            l[:] = np.inf                                                       # a tree whose bounds are all +inf
        covers.append((f, l, rng.uniform(0., 1., (n, d['n_dual'])), rng.uniform(0., 1., n)))
    ref = sr.Search(d, K, cap, ds.row_cap)
    x0s = rng.uniform(-1., 1., (K, d['nx']))
    ref.begin(x0s, covers)
    ds.begin(x0s, _cover_arrays(covers))
    _same_state(ds, ref, (name, K, 'begin'), trees=range(min(K, 7)))
    sizes_seen, took_part = [], set()
    for q in range(3):
        B = _round(ds, ref, d, width, tol, q % 2 == 0, rng, (name, K, width, q))
        sizes_seen.append(B)
        took_part |= set(ref.batch['tree'])
        sr.compare_dicts(ref.results(), ds.results(), what=(name, K, 'round', q))
        if B == 0:
            break
    _same_state(ds, ref, (name, K, width, tol), trees=list(range(min(K, 14))) + [K - 1])
    res = ref.results()
    assert sizes_seen[0] > 0 and (K < 5 or (res['state'] & sr.DONE).any())
    if K >= 7:
        assert (res['state'] & sr.OVERFLOW).any() and res['uncertified'].any()
    if K > SCAN_CHUNK:
        assert K - 1 in took_part and res['solves'][K - 1] > 0                  # the tree behind the carry took part


def test_complete_pick_then_failed_record_weak_rows_and_guards():
    # one round of three trees: a COMPLETE pick followed by one that only the lowered cutoff prunes; a FAILED record in the middle
    # of a tree's picks; WEAK records whose dual objective becomes -inf -- and no other entry of the pool is written: every row is
    # a guard before the round
    ds, d = _search('random_mld_t5', 3, 16, 40)
    nfix = d['nfix']
    rng = np.random.default_rng(5)
    full = np.zeros((3, nfix), np.int8)
    full[1, -1] = full[2, -2] = 1
    free = np.full((3, nfix), -1, np.int8)
    free[:, 0] = [0, 1, 1]
    free[2, 1] = 0
    covers = [(full, np.array([.1, .2, .3]), None, None), (free, np.array([.1, .2, .3]), None, None), (free.copy(), np.array([.3, .2, .1]), None, None)]
    ref = sr.Search(d, 3, 16, 40)
    x0s = rng.uniform(-1., 1., (3, d['nx']))
    ref.begin(x0s, covers)
    zeros = lambda n: (np.zeros((n, d['n_dual'])), np.zeros(n))
    ds.begin(x0s, _cover_arrays([(f, l) + zeros(len(l)) for f, l, _, _ in covers]))
    guard = dict(obj=np.full(40, -7.), dual_obj=np.full(40, -7.), status=np.full(40, -7, np.int32), iters=np.full(40, -7, np.int32),
                 primal=np.full((40, d['n_primal']), -7.), dual=np.full((40, d['n_dual']), -7.))
    ds.rows(0, 40, guard)                                                       # (the covers' rows 0 .. 8 included: nothing reads them here)
    vertex = br.POLISHED_BIT | 4
    plan = lambda batch: {0: (0, 1., vertex), 1: (0, 1.5, vertex), 2: (0, .5, vertex),        # incumbent 1, pruned by it, incumbent .5
                          3: (0, 1., vertex), 4: (3, 1., 4), 5: (0, 1., vertex),               # branched, FAILED, never consumed
                          6: (1, np.inf, br.WEAK_BIT | 4), 7: (1, np.inf, br.WEAK_BIT | br.UNCERTIFIED_BIT | 4), 8: (1, np.inf, 4)}
    # (the device's trees began with rows 0 .. 8 of zeros as their covers' dual rows; the restatement's with none: rows are compared below)
    B = ref.select(8, 0., True)
    assert ds.select(8, 0., True) == B == 9
    got = ds.batch()
    assert got['row0'] == 9 and np.array_equal(got['tree'], ref.batch['tree']) and np.array_equal(got['node'], ref.batch['node'])
    assert np.array_equal(got['node'], [0, 1, 2, 0, 1, 2, 2, 1, 0])
    rec = sr.synthetic_records(d, ref.batch['fix'], rng, plan=plan(None))
    ref.put_records(rec)
    ds.put_records(rec)
    ref.consume(0.)
    ds.consume(0.)
    t = [ds.tree(k) for k in range(3)]
    assert t[0]['inc'] == 2 and t[0]['ub'] == .5 and t[0]['solves'] == 3 and br.same_bits(t[0]['lb'][:3], np.array([1., 1.5, .5]))
    assert t[1]['state'] == sr.FAILED and t[1]['solves'] == 1 and t[1]['n'] == 5 and t[1]['lb'][1] == .2
    assert t[2]['uncertified'] == 1 and t[2]['unc_lb'] == .2 and t[2]['solves'] == 3 and np.all(np.isinf(t[2]['lb'][:3]))
    for k in range(3):
        r = ref.tree(k)
        r['row'] = np.where(r['row'] >= 0, r['row'] + 9, np.arange(len(r['row'])) + 3 * k).astype(np.int32)       # (rows behind the covers' nine)
        r['wrow'] = np.where(r['wrow'] >= 0, r['wrow'] + 9, -1).astype(np.int32)
        r['inc_row'] = r['inc_row'] + 9 if r['inc_row'] >= 0 else -1
        sr.compare_tree(r, t[k], what=k)
    pool = ds.rows(0, 40)
    want = {k: v.copy() for k, v in guard.items()}
    for k in sr.RECORD_KEYS:
        want[k][9:18] = rec[k]
    want['dual_obj'][[15, 16]] = -np.inf                                        # the two WEAK records, and nothing else
    for k in sr.RECORD_KEYS:
        assert br.same_bits(want[k], pool[k]), k


def test_overflow_leaves_the_slab_as_it_was_and_row_cap_refuses_the_round():
    from warm_start_hmpc_amd.search import SearchTooBig
    cap = 9
    ds, d = _search('random_mld_t5', 2, cap, 2 * (cap - 1) + 3)
    rng = np.random.default_rng(11)
    covers = []
    for k in range(2):
        f, l = sr.random_cover(d, cap - 1, rng, ties=False, infs=False)
        f[:, -1] = -1                                                           # (every leaf has a free binary)
        covers.append((f, l, rng.uniform(0., 1., (cap - 1, d['n_dual'])), rng.uniform(0., 1., cap - 1)))
    ref = sr.Search(d, 2, cap, ds.row_cap)
    x0s = np.zeros((2, d['nx']))
    ref.begin(x0s, covers)
    ds.begin(x0s, _cover_arrays(covers))
    before = [ds.tree(k) for k in range(2)]
    # row_cap: 16 rows hold the covers, 3 are left; a round of 2 x 2 picks is refused with nothing changed ...
    with pytest.raises(sr.TooBig):
        ref.select(2, 0., True)
    with pytest.raises(SearchTooBig, match='row_cap'):
        ds.select(2, 0., True)
    for k in range(2):
        after = ds.tree(k)
        for key in before[k]:
            assert br.same_bits(np.asarray(before[k][key]), np.asarray(after[key])), (k, key)
    assert ds.qp.lib.hmpc_search_consume(ds._s, 0., None) == -1 and b'no round is staged' in ds.qp.lib.hmpc_last_error()
    # ... one of 2 x 1 fits.  Every record would branch; a slab of cap - 1 nodes has no room for two children: OVERFLOW at the
    # first pick, and the whole slab (all node_cap entries) and every scalar but the state are as before the pick
    vertex = br.POLISHED_BIT | 3
    B = _round(ds, ref, d, 1, 0., True, rng, 'overflow', plan=lambda batch: {0: (0, 1., vertex), 1: (0, 1., vertex)})
    assert B == 2
    for k in range(2):
        after = ds.tree(k)
        assert after.pop('state') == sr.OVERFLOW and before[k].pop('state') == 0
        for key in before[k]:
            assert br.same_bits(np.asarray(before[k][key]), np.asarray(after[key])), (k, key)
    _same_state(ds, ref, 'overflow')
    assert ds.select(1, 0., True) == 0 == ref.select(1, 0., True)               # stopped trees take no part


def test_arguments_that_need_a_handle_are_refused():
    from helpers import random_mld, _NoBackend
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP, _Result
    ctrl, qp, d = _backend('random_mld_t5')
    lib = qp.lib
    out = ctypes.c_void_p()
    for K, node_cap, row_cap in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        assert lib.hmpc_search_create(qp.handle, K, node_cap, row_cap, ctypes.byref(out)) == -1 and not out.value
    assert lib.hmpc_search_create(qp.handle, 2, 8, 8, None) == -1
    ds, _ = _search('random_mld_t5', 2, 8, 8)
    x0s = np.zeros((2, d['nx']))
    B = ctypes.c_int32(-7)
    assert lib.hmpc_search_select(ds._s, 8, 0., 1, ctypes.byref(B), None) == -1 and b'no step has begun' in lib.hmpc_last_error()
    count = np.array([3, 9], np.int32)                                          # a cover beyond its slab
    fix, lb = np.full((12, d['nfix']), -1, np.int8), np.zeros(12)
    assert lib.hmpc_search_begin(ds._s, x0s.ctypes.data, count.ctypes.data, fix.ctypes.data, lb.ctypes.data, None, None) == -1
    assert b'node_cap' in lib.hmpc_last_error()
    count = np.array([5, 5], np.int32)                                          # covers whose rows are beyond the pool
    dual, dobj = np.zeros((10, d['n_dual'])), np.zeros(10)
    assert lib.hmpc_search_begin(ds._s, x0s.ctypes.data, count.ctypes.data, fix.ctypes.data, lb.ctypes.data, dual.ctypes.data, dobj.ctypes.data) == -1
    assert b'row_cap' in lib.hmpc_last_error()
    ds.begin(x0s)
    for width in (0, 65):
        assert lib.hmpc_search_select(ds._s, width, 0., 1, ctypes.byref(B), None) == -1 and B.value == -7
    assert lib.hmpc_search_consume(ds._s, 0., None) == -1 and b'no round is staged' in lib.hmpc_last_error()
    assert ds.select(8) == 2
    assert lib.hmpc_search_put_records(ds._s, 2, ctypes.byref(_Result())) == -1 and b'required' in lib.hmpc_last_error()
    # a problem without binaries has nothing to search
    import os
    mld, objective, _ = random_mld(nx=6, nuc=2, nub=0, seed=3)
    plain = HybridModelPredictiveController(mld, 5, objective, None, backend=_NoBackend())
    old = os.environ.get('HMPC_JIT')
    os.environ['HMPC_JIT'] = '0'
    try:
        none = HipBatchedQP(plain.problem_data())
    finally:
        if old is None:
            del os.environ['HMPC_JIT']
        else:
            os.environ['HMPC_JIT'] = old
    assert lib.hmpc_search_create(none.handle, 2, 8, 8, ctypes.byref(out)) == -1 and b'no binaries' in lib.hmpc_last_error() and not out.value


# ---- whole searches ---------------------------------------------------------------------------------------------------------------
def _solver(qp, ref, handdown):
    """The restatement's callback: the same handle's solve_batch on the same batches in the same order; a node receives its
    parent's record from the restatement's own pool (as hmpc_solve_batch does it: the hand-down only where a node receives one)."""
    def solve(x0, fix, warm):
        w = None
        if handdown and (warm >= 0).any():
            w = (ref.pool['primal'][:ref.row0], ref.pool['dual'][:ref.row0], warm)
        return br.as_word_records(qp.solve_batch(x0, fix, warm=w))
    return solve


@pytest.mark.parametrize('handdown', [False, True])
@pytest.mark.parametrize('width', [1, 8])
def test_cart_pole_searches_match_the_restatement_to_the_bit(width, handdown):
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, qp, d = _backend('cart_pole_t20')
    x0s = np.array([X0, X0 * .5, INFEASIBLE])
    ref = sr.Search(d, 3, 4096, 4096)
    ref.begin(x0s)
    rounds, launched = ref.run(_solver(qp, ref, handdown), width, 0., handdown)
    # node_cap and row_cap: twice what the restatement's own run needs
    ds = DeviceSearch(ctrl, 3, node_cap=2 * max(len(t.lb) for t in ref.trees), row_cap=2 * ref.row0)
    ds.begin(x0s)
    assert ds.run(width, 0., handdown) == (rounds, launched)
    want, got = ref.results(), ds.results()
    print('width %d handdown %d: %d rounds, %d nodes, solves %s, leaves %s, cost %s' % (width, handdown, rounds, launched, got['solves'], got['leaves'], got['cost']))
    sr.compare_dicts(want, got, what=(width, handdown))
    assert np.all(got['state'] & sr.DONE) and not np.any(got['state'] & (sr.FAILED | sr.OVERFLOW))      # a condition, not a measurement
    assert np.array_equal(got['state'], [sr.DONE | sr.INCUMBENT, sr.DONE | sr.INCUMBENT, sr.DONE])
    assert np.isfinite(got['cost'][:2]).all() and np.isinf(got['cost'][2]) and np.isnan(got['u0'][2]).all() and got['solves'][0] > 20
    sr.compare_dicts(ref.leaves(), ds.leaves_flat(), what=(width, handdown, 'leaves'))
    for k in range(3):
        sr.compare_tree(ref.tree(k), ds.tree(k), what=(width, handdown, 'tree', k))
    if handdown:
        assert (ds.rows(0, ref.row0)['iters'] & br.HANDED_BIT).any()           # (records were handed down, and some verified)


def test_feedforward_many_is_interchangeable_with_the_numpy_driver():
    from warm_start_hmpc_amd.batched import BatchedMPC
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, qp, d = _backend('cart_pole_t20')
    x0s = np.array([X0, INFEASIBLE])
    py = BatchedMPC(ctrl).feedforward_many(x0s, None, frontier_width=8)
    dv = DeviceSearch(ctrl, 2, node_cap=1024, row_cap=2048).feedforward_many(x0s, None, frontier_width=8, handdown=False)
    for a, b in zip(py, dv):
        assert a['objective'] == b['objective'] and a['solves'] == b['solves'] and a['rounds'] == b['rounds']
        assert np.array_equal(a['leaves'].fix, b['leaves'].fix) and br.same_bits(a['leaves'].lb, b['leaves'].lb)
        assert br.same_bits(a['leaves'].dual, b['leaves'].dual) and br.same_bits(a['leaves'].dobj, b['leaves'].dobj)
        if a['ub'] is not None:
            assert br.same_bits(a['x'][1], b['x'][1]) and br.same_bits(a['uc'][0], b['uc'][0]) and np.array_equal(np.rint(a['ub']), b['ub'])
        else:
            assert b['ub'] is None and b['x'] is None


def test_three_closed_loop_steps_walk_the_walk_of_the_numpy_driver():
    # run -> leaves -> shift_batch -> begin, with the disturbances of the reference's published run; the bounds are those of
    # test_fleet_walks_the_walk_of_the_numpy_driver, for the reason it gives.  Without the hand-down a round of the device search is
    # the very batch the numpy driver solves: the same kernel variant for every node
    from helpers import load_fixture
    from warm_start_hmpc_amd.batched import BatchedMPC
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, qp, d = _backend('cart_pole_t20')
    K, steps = 4, 3
    errors = load_fixture('reference_closed_loop')['errors_0003'][:K, :steps]
    dv = DeviceSearch(ctrl, K, node_cap=1024, row_cap=4096).closed_loop(X0, steps, errors, frontier_width=8, handdown=False)
    py = BatchedMPC(ctrl).closed_loop(X0, steps, seeds=tuple(range(K)), frontier_width=8, errors=errors)
    np.testing.assert_allclose(dv['costs'], np.array(py['costs']), rtol=1e-9, atol=1e-12)
    assert np.array_equal(dv['len_ws'], np.array(py['len_ws']))
    assert np.array_equal(dv['reopened'], np.array(py['reopened']))
    assert dv['steps'] == K * steps
