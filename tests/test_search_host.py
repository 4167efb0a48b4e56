"""The device-resident search (include/hmpc_search.h) without a GPU: the per-tree functions of csrc/hmpc_search.h -- what the kernels'
lanes run -- walked serially over K trees (tests/host/search_driver.cpp) under AddressSanitizer and UBSan, held to the numpy
restatement of tests/search_reference.py (integers exactly, floats bit for bit) on full cold searches over oracle-solved records and
on synthetic rounds, and to BatchedMPC.feedforward_many on the oracle backend; two planted defects, each of which the comparison
must catch; the C ABI's new entries: named by the header as the binding names them, rejecting bad arguments without a GPU, and no
CPU answer where there is none."""
import ctypes
import os
import re

import numpy as np
import pytest

import branch_reference as br
import search_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.fixture(scope='module', autouse=True)
def no_error_text_left_behind():
    """As in test_branch_host.py: the refusals provoked here leave their text in hmpc_last_error; a successful call that needs no GPU
    ends the module with the empty text other modules start from."""
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
    directory = tmp_path_factory.mktemp('search')
    return sr.build_driver(directory), directory


EMPTY = dict(obj=np.zeros(0), dual_obj=np.zeros(0), status=np.zeros(0, np.int32), iters=np.zeros(0, np.int32), primal=np.zeros((0, 1)), dual=np.zeros((0, 1)))


def _states(name, x0):
    """Three trees per problem: the state of branch_reference.solved, a second one, and one far outside (cart-pole: infeasible)."""
    if name == 'cart_pole_t10':
        return np.array([x0, x0 * .5, [0., 0., 5., 0.]])
    return np.array([x0, x0 * .5, x0 * 1.5])


@pytest.fixture(scope='module')
def cold_searches():
    """Per problem and width: the restatement's full cold search of three trees with oracle-solved records, its rounds recorded."""
    memo = {}

    def get(name, width):
        if (name, width) not in memo:
            ctrl, x0, _, _ = br.solved(name)
            d = br.dims_of(ctrl.problem_data())
            x0s = _states(name, x0)
            ref = sr.Search(d, len(x0s), node_cap=2048, row_cap=8192)
            ref.begin(x0s)
            rounds, batches = [], []

            def solve(x0b, fix, warm):
                rec = br.as_word_records(ctrl.qp.solve_batch(x0b, fix))
                rounds.append(rec)
                batches.append({k: ref.batch[k].copy() for k in ('tree', 'node', 'warm')})
                return rec
            ref.run(solve, width, 0., True)
            memo[name, width] = (ctrl, d, x0s, ref, rounds, batches)
        return memo[name, width]
    return get


@pytest.mark.parametrize('name', ['cart_pole_t10', 'random_mld'])
@pytest.mark.parametrize('width', [1, 8])
def test_cold_search_over_oracle_records_matches_restatement(driver, cold_searches, name, width):
    ctrl, d, x0s, ref, rounds, batches = cold_searches(name, width)
    K = len(x0s)
    assert len(rounds) >= 5 and sum(len(r['obj']) for r in rounds) >= 20
    need = max(len(t.lb) for t in ref.trees)
    trees, got_batches, dual_obj = sr.run_driver(*driver, d, K, need, None, rounds + [EMPTY], width, 0., True)
    assert len(got_batches) == len(batches)
    for q, (a, b) in enumerate(zip(batches, got_batches)):
        sr.compare_dicts(a, b, what=(name, 'round', q))
    for k in range(K):
        sr.compare_tree(ref.tree(k), trees[k], what=(name, 'tree', k))
    assert br.same_bits(dual_obj, ref.pool['dual_obj'][:ref.row0])
    res = ref.results()
    assert np.all(res['state'] & sr.DONE) and not np.any(res['state'] & (sr.FAILED | sr.OVERFLOW))
    assert np.isfinite(res['cost'][0]) and (name != 'cart_pole_t10' or np.isinf(res['cost'][2]))
    assert any(b['warm'].max(initial=-1) >= 0 for b in batches)                  # (rows are handed down)


@pytest.mark.parametrize('name', ['cart_pole_t10', 'random_mld'])
def test_cold_search_is_the_search_of_the_numpy_driver(cold_searches, name):
    from warm_start_hmpc_amd.batched import BatchedMPC
    ctrl, d, x0s, ref, rounds, batches = cold_searches(name, 8)
    py = BatchedMPC(ctrl).feedforward_many(x0s, None, frontier_width=8, tol=0.)
    res, lv = ref.results(), ref.leaves()
    for k, r in enumerate(py):
        assert br.same_bits(np.float64(r['objective']), res['cost'][k]), (k, r['objective'], res['cost'][k])
        assert r['solves'] == res['solves'][k]
        if r['ub'] is not None:
            assert np.array_equal(np.rint(r['ub']).astype(np.int8).reshape(-1), res['binaries'][k])
            assert br.same_bits(r['x'][1], res['x1'][k]) and br.same_bits(np.concatenate((r['uc'][0], r['ub'][0])), res['u0'][k])
        else:
            assert res['state'][k] == sr.DONE
        m = lv['owner'] == k
        assert np.array_equal(r['leaves'].fix, lv['fix'][m]) and br.same_bits(r['leaves'].lb, lv['lb'][m])
        assert br.same_bits(r['leaves'].dual, lv['dual'][m]) and br.same_bits(r['leaves'].dobj, lv['dual_obj'][m])


def _synthetic_case(d, seed, K=4, n=12, width=3, rounds=3, tol=0., node_cap=64):
    """Covers with ties and +inf bounds, then `rounds` rounds of synthetic records drawn for the restatement's batches."""
    rng = np.random.default_rng(seed)
    covers = [sr.random_cover(d, n if k != 1 else 0, rng) for k in range(K)]
    ref = sr.Search(d, K, node_cap, 4096)
    ref.begin(np.zeros((K, d['nx'])), [(f, l, None, None) for f, l in covers])
    recs, batches = [], []
    for _ in range(rounds):
        B = ref.select(width, tol, True)
        if B == 0:
            recs.append(EMPTY)                                                  # (the walk under test has to end here too)
            break
        rec = sr.synthetic_records(d, ref.batch['fix'], rng)
        ref.put_records(rec)
        ref.consume(tol)
        recs.append(rec)
        batches.append({k: ref.batch[k].copy() for k in ('tree', 'node', 'warm')})
    return covers, ref, recs, batches


SHAPE = dict(nx=3, nu=4, nub=3, T=5, h=np.zeros(4), h_Tm1=np.zeros(6), Q=np.zeros((3, 1)), R=np.zeros((2, 1)), Q_T=np.zeros((3, 1)))


@pytest.mark.parametrize('tol', [0., .5])
@pytest.mark.parametrize('width', [1, 3, 64])
def test_synthetic_rounds_match_restatement(driver, width, tol):
    d = br.dims_of(SHAPE)
    covers, ref, recs, batches = _synthetic_case(d, 7 + width, width=width, tol=tol, rounds=4)
    trees, got, dual_obj = sr.run_driver(*driver, d, 4, 64, covers, recs, width, tol, True)
    assert len(got) == len(batches) >= 3
    for q, (a, b) in enumerate(zip(batches, got)):
        sr.compare_dicts(a, b, what=('round', q))
    for k in range(4):
        sr.compare_tree(ref.tree(k), trees[k], what=('tree', k))
    assert br.same_bits(dual_obj, ref.pool['dual_obj'][:ref.row0]) and np.isneginf(dual_obj).any()


def _complete_then_pruned(d):
    """One tree of two complete leaves A (bound .1) and B (.2) picked in one round: A's record is an incumbent of cost 1, B's a
    complete node of cost 1.5 -- only the cutoff A has just lowered prunes it."""
    fix = np.zeros((2, d['nfix']), np.int8)
    fix[1, -1] = 1
    covers = [(fix, np.array([.1, .2]))]
    rec = sr.synthetic_records(d, fix, np.random.default_rng(0), plan={0: (0, 1., br.POLISHED_BIT | 9), 1: (0, 1.5, br.POLISHED_BIT | 9)})
    return covers, rec


def _run_both(driver, d, covers, recs, width, defect, node_cap=16):
    K = len(covers)
    ref = sr.Search(d, K, node_cap, 64)
    ref.begin(np.zeros((K, d['nx'])), [(f, l, None, None) for f, l in covers])
    for rec in recs:
        assert ref.select(width, 0., True) == len(rec['obj'])
        ref.put_records(rec)
        ref.consume(0.)
    trees, got, _ = sr.run_driver(*driver, d, K, node_cap, covers, recs, width, 0., True, defect=defect)
    return ref, trees


def test_a_complete_pick_lowers_the_cutoff_of_the_next_pick(driver):
    d = br.dims_of(SHAPE)
    covers, rec = _complete_then_pruned(d)
    ref, trees = _run_both(driver, d, covers, [rec], 8, 0)
    sr.compare_tree(ref.tree(0), trees[0])
    assert trees[0]['inc'] == 0 and trees[0]['ub'] == 1. and trees[0]['solves'] == 2 and br.same_bits(trees[0]['lb'], np.array([1., 1.5]))


@pytest.mark.parametrize('defect', ['stale_cutoff', 'unstable_ties'])
def test_planted_defects_fail_the_comparison(driver, defect):
    d = br.dims_of(SHAPE)
    if defect == 'stale_cutoff':
        covers, rec = _complete_then_pruned(d)
        recs, width = [rec], 8
    else:                                                                       # four equal bounds, two picks: nodes 0 and 1, in that order
        fix = np.full((4, d['nfix']), -1, np.int8)
        fix[:, :2] = [[0, 0], [0, 1], [1, 0], [1, 1]]
        covers = [(fix, np.full(4, .25))]
        recs, width = [sr.synthetic_records(d, fix[:2], np.random.default_rng(1), plan={0: (0, 1., 3), 1: (0, 1.25, 3)})], 2
    ref, good = _run_both(driver, d, covers, recs, width, 0)
    sr.compare_tree(ref.tree(0), good[0])
    ref, bad = _run_both(driver, d, covers, recs, width, {'stale_cutoff': 1, 'unstable_ties': 2}[defect])
    with pytest.raises(AssertionError):
        sr.compare_tree(ref.tree(0), bad[0], what=defect)
    # ... and the restatement with the same defect planted walks the defective walk
    twin = sr.Search(d, 1, 16, 64, defect=defect)
    twin.begin(np.zeros((1, d['nx'])), [(covers[0][0], covers[0][1], None, None)])
    twin.select(width, 0., True)
    twin.put_records(recs[0])
    twin.consume(0.)
    sr.compare_tree(twin.tree(0), bad[0], what=defect)


def test_overflow_and_failed_records_stop_a_tree(driver):
    d = br.dims_of(SHAPE)
    fix = np.full((3, d['nfix']), -1, np.int8)
    fix[:, 0] = [0, 1, 1]
    fix[2, 1] = 0
    covers = [(fix, np.array([.1, .2, .3]))] * 2
    rng = np.random.default_rng(2)
    branch = (0, 1., br.POLISHED_BIT | 5)
    rec = sr.synthetic_records(d, np.vstack((fix, fix)), rng, plan={0: branch, 1: branch, 2: branch, 3: branch, 4: (2, 1., 5), 5: branch})
    ref, trees = _run_both(driver, d, covers, [rec], 3, 0, node_cap=6)        # tree 0: 3 + 2 children fit, the second branch does not
    for k in range(2):
        sr.compare_tree(ref.tree(k), trees[k], what=k)
    assert trees[0]['state'] == sr.OVERFLOW and trees[0]['n'] == 5 and trees[0]['solves'] == 1
    assert trees[1]['state'] == sr.FAILED and trees[1]['n'] == 5 and trees[1]['solves'] == 1


def test_header_and_binding_name_the_same_symbols_and_states():
    from warm_start_hmpc_amd import qp_backend
    header = open(os.path.join(ROOT, 'include', 'hmpc_search.h')).read()
    declared = re.findall(r'^int\s+(hmpc_[a-z_]+)\s*\(', header, re.M)
    assert tuple(declared) == qp_backend.EXPORTED_SEARCH_SYMBOLS
    assert not set(declared) & set(qp_backend.EXPORTED_SYMBOLS)
    states = dict((name.lower(), int(v, 16)) for name, v in re.findall(r'#define HMPC_SEARCH_([A-Z_]+)\s+(0x[0-9a-fA-F]+)\b', header))
    assert states == qp_backend.SEARCH_STATES == dict(done=sr.DONE, incumbent=sr.INCUMBENT, failed=sr.FAILED, overflow=sr.OVERFLOW)
    lib = qp_backend.load_library()
    for name in declared:
        assert getattr(lib, name) is not None
    # the header of the kernels' key is not touched by this one
    assert 'hmpc_search' not in open(os.path.join(ROOT, 'include', 'hmpc.h')).read()


def test_invalid_arguments_are_rejected_without_touching_the_gpu():
    from warm_start_hmpc_amd.qp_backend import load_library
    lib = load_library()
    out = ctypes.c_void_p()
    B = ctypes.c_int32(-7)
    n = ctypes.c_int32(0)
    for K, node_cap, row_cap in ((0, 16, 16), (4, 0, 16), (4, 16, 0), (-1, 16, 16)):
        assert lib.hmpc_search_create(None, K, node_cap, row_cap, ctypes.byref(out)) == -1 and not out.value
        assert b'must be positive' in lib.hmpc_last_error()
    assert lib.hmpc_search_create(None, 4, 16, 16, ctypes.byref(out)) == -1 and b'null handle' in lib.hmpc_last_error() and not out.value
    assert lib.hmpc_search_create(None, 4, 16, 16, None) == -1
    assert lib.hmpc_search_begin(None, None, None, None, None, None, None) == -1 and b'null' in lib.hmpc_last_error()
    for width in (0, 65, -1):
        assert lib.hmpc_search_select(None, width, 0., 1, ctypes.byref(B), None) == -1 and b'width' in lib.hmpc_last_error()
    assert lib.hmpc_search_select(None, 8, 0., 1, ctypes.byref(B), None) == -1 and b'null' in lib.hmpc_last_error()
    assert B.value == -7
    assert lib.hmpc_search_consume(None, 0., None) == -1
    assert lib.hmpc_search_put_records(None, 1, None) == -1
    assert lib.hmpc_search_run(None, 8, 0., 1, 0, None, None, None) == -1
    assert lib.hmpc_search_results(None, *[None] * 8) == -1
    assert lib.hmpc_search_leaves(None, ctypes.byref(n), *[None] * 6) == -1
    assert lib.hmpc_search_batch(None, None, None, None, None, None) == -1
    assert lib.hmpc_search_get_batch(None, 1, *[None] * 5) == -1 and lib.hmpc_search_tree(None, 0, *[None] * 7) == -1
    assert lib.hmpc_search_rows(None, 0, 1, None, 0) == -1
    assert lib.hmpc_search_destroy(None) == 0


@pytest.mark.skipif(_has_gpu(), reason='only meaningful on a box without a GPU')
def test_product_path_fails_loudly_without_gpu():
    from helpers import make_controller
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    from warm_start_hmpc_amd.search import DeviceSearch
    with pytest.raises(RuntimeError, match='HIP backend'):
        DeviceSearch(make_controller('cart_pole_with_walls', T=10, backend='oracle'), 2)
    with pytest.raises(RuntimeError, match=r'\(-2\)'):                           # no handle without a device, so no search either
        HipBatchedQP(make_controller('cart_pole_with_walls', T=10, backend='oracle').problem_data())
