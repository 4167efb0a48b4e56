"""hmpc_search_advance on the device (the retain, offsets, stage and adopt kernels of csrc/hmpc_search.hip around hmpc_launch_shift),
held to the step boundary the same handle's existing entries give -- results -> leaves -> hmpc_shift_batch -> filter on keep ->
begin --, integers exactly, floats bit for bit: both paths run the same shift kernel on the same per-leaf inputs.  Synthetic trees
in every state an advance tells apart (tests/advance_reference.py), under both shift kernels; the refusals, which change nothing;
three closed-loop steps of the cart-pole with walls, resident against the host path."""
import os

import numpy as np
import pytest

import advance_reference as ar
import branch_reference as br
import search_reference as sr
from test_gpu_branch import _backend
from test_search_advance_host import SIZES, STATES, CASES

pytestmark = pytest.mark.gpu
X0 = np.array([0., 0., 1., 0.])                                                # (tests/test_gpu_search.py)
INFEASIBLE = np.array([0., 0., 5., 0.])
_MAPS = {}


def _ready(name):
    """(ctrl, qp, d, BatchedMPC) with the shift's maps uploaded."""
    from warm_start_hmpc_amd.batched import BatchedMPC
    ctrl, qp, d = _backend(name)
    if name not in _MAPS:
        _MAPS[name] = BatchedMPC(ctrl)
    return ctrl, qp, d, _MAPS[name]


def _begin(ds, d, x0s, covers, duals):
    """begin from covers (fix, lb) with the dual rows `duals` [(dual, dual_obj)] or, duals None, without rows (row = -1)."""
    count = np.array([len(l) for _, l in covers], np.int32)
    fix = np.ascontiguousarray(np.concatenate([f for f, _ in covers]), np.int8)
    lb = np.ascontiguousarray(np.concatenate([l for _, l in covers]), np.float64)
    x0s = np.ascontiguousarray(x0s, np.float64)
    dual = dobj = None
    if duals is not None:
        dual = np.ascontiguousarray(np.concatenate([a for a, _ in duals]), np.float64)
        dobj = np.ascontiguousarray(np.concatenate([b for _, b in duals]), np.float64)
    ds._check(ds.qp.lib.hmpc_search_begin(ds._s, x0s.ctypes.data, count.ctypes.data, fix.ctypes.data, lb.ctypes.data,
                                          None if dual is None else dual.ctypes.data, None if dobj is None else dobj.ctypes.data))


def _follow(ds):
    def follow(width, B, rec):
        assert ds.select(width, 0., True) == B
        if B:
            ds.put_records(rec)
            ds.consume(0.)
    return follow


def _expected(ds, x0s, e0, x0_next=None):
    """What an advance must leave, from the existing entries of the same handle: results(), leaves_flat(), qp.shift_batch, then the
    filter on keep.  Returns dict trees (as Search.tree), dual, dual_obj (the first B rows of the next pool), cover, reopened,
    x0_next, and the shift's outputs for the kept leaves (for the restatement that walks along)."""
    K = ds.K
    res, lv = ds.results(), ds.leaves_flat()
    adv = res['state'] == ar.ADVANCES
    u0 = np.where(adv[:, None], res['u0'], 0.)
    m = adv[lv['owner']]
    out = ds.qp.shift_batch(lv['owner'][m], x0s, u0, e0, lv['fix'][m], lv['lb'][m], lv['dual'][m], lv['dual_obj'][m])
    keep = out['keep']
    owner, opened = lv['owner'][m][keep], (out['reopened'] | ~lv['has_dual'][m])[keep]
    fix, lb = out['fix'][keep], out['lb'][keep]
    trees, b = [], 0
    for k in range(K):
        n = int((owner == k).sum())
        assert np.all(owner[b:b + n] == k)
        trees.append(dict(n=n, inc=-1, inc_row=-1, solves=0, uncertified=0, state=0, ub=np.float64(np.inf), unc_lb=np.float64(np.inf),
                          fix=fix[b:b + n], lb=lb[b:b + n], row=np.arange(b, b + n, dtype=np.int32), wrow=np.full(n, -1, np.int32), alive=np.ones(n, np.uint8)))
        b += n
    return dict(trees=trees, dual=out['dual'][keep], dual_obj=out['dual_obj'][keep], B=b,
                cover=np.array([t['n'] for t in trees], np.int32), reopened=np.array([int(opened[owner == k].sum()) for k in range(K)], np.int32),
                x0_next=np.array(x0_next) if x0_next is not None else np.where(adv[:, None], res['x1'] + e0, x0s),
                shift=dict(fix_out=fix, lb_out=lb, flags=(1 | 2 * out['reopened'][keep]).astype(np.uint8), dual=out['dual'][keep], dual_obj=out['dual_obj'][keep]))


def _same_after(ds, want, what):
    for k, t in enumerate(want['trees']):
        sr.compare_tree(t, ds.tree(k), what=(what, 'tree', k))
    B = want['B']
    got = ds.rows(0, B)
    assert br.same_bits(got['dual'], want['dual']) and br.same_bits(got['dual_obj'], want['dual_obj']), what
    assert ds.batch(device=True)['row0'] == B


def _snapshot(ds):
    pool = ds.rows(0, ds.row_cap)
    return [ds.tree(k) for k in range(ds.K)], pool, ds.results()


def _unchanged(ds, snap, what):
    trees, pool, res = snap
    for k in range(ds.K):
        now = ds.tree(k)
        for key in trees[k]:
            assert br.same_bits(np.asarray(trees[k][key]), np.asarray(now[key])), (what, k, key)
    now = ds.rows(0, ds.row_cap)
    for key in pool:
        assert br.same_bits(pool[key], now[key]), (what, key)
    sr.compare_dicts(res, ds.results(), what=what)


@pytest.mark.parametrize('shift_rows', [None, '0'])
@pytest.mark.parametrize('name,case,with_rows', [('random_mld_t5', 'sizes', True), ('random_mld_t5', 'sizes', False), ('cart_pole_t16', 'sizes', True),
                                                 ('random_mld_t5', 'states', True), ('cart_pole_t16', 'states', False), ('cart_pole_t16', 'one', True)])
def test_synthetic_states_advance_as_the_host_entries_do(monkeypatch, name, case, with_rows, shift_rows):
    # trees of 1, 63, 64, 65 and 129 nodes with dead nodes in between, children that share their parent's row, trees without
    # incumbent, with leaves that all disagree, FAILED, OVERFLOW; covers without rows (row < 0: the row of zeros); two advances in a
    # row: the second reads the pool the first wrote.  HMPC_SHIFT_ROWS is read per launch: both shift kernels
    from warm_start_hmpc_amd.search import DeviceSearch
    if shift_rows is None:
        monkeypatch.delenv('HMPC_SHIFT_ROWS', raising=False)
    else:
        monkeypatch.setenv('HMPC_SHIFT_ROWS', shift_rows)
    ctrl, qp, d, _ = _ready(name)
    specs, node_cap = CASES[case]
    K = len(specs)
    rng = np.random.default_rng(len(name) + 3 * with_rows)
    ds = DeviceSearch(ctrl, K, node_cap=node_cap, row_cap=2048)
    covers, u0b = ar.make_covers(d, specs, rng, node_cap)
    duals = [(rng.uniform(0., 1., (len(l), d['n_dual'])), rng.uniform(0., 1., len(l))) for _, l in covers] if with_rows else None
    x0s = rng.uniform(-1., 1., (K, d['nx']))
    ref = ar.Search(d, K, node_cap, ds.row_cap)
    ref.begin(x0s, [(f, l) + (duals[k] if with_rows else (None, None)) for k, (f, l) in enumerate(covers)])
    _begin(ds, d, x0s, covers, duals)
    for step in range(2):
        ar.run_step(ref, d, specs, u0b, rng, follow=_follow(ds))
        sr.compare_dicts(ref.results(), ds.results(), what=(name, case, step, 'the step ended'))
        e0 = rng.uniform(-.1, .1, (K, d['nx'])) if step == 0 else None
        xn = rng.uniform(-1., 1., (K, d['nx'])) if step == 1 else None
        want = _expected(ds, ref.x0, np.zeros((K, d['nx'])) if e0 is None else e0, xn)
        got = ds.advance(e0, xn)
        print('%s %s rows %s kernel %s step %d: B %d cover %s reopened %s' % (name, case, with_rows, shift_rows, step, want['B'], got['cover'], got['reopened']))
        assert np.array_equal(got['cover'], want['cover']) and np.array_equal(got['reopened'], want['reopened'])
        _same_after(ds, want, (name, case, with_rows, shift_rows, step))
        # the restatement walks along on the shift's outputs: its retain and staging order are those of the device
        staged = ref.advance(lambda st: want['shift'], e0, xn)
        assert staged['B'] == want['B'] and np.array_equal(staged['cover'], got['cover']) and np.array_equal(staged['reopened'], got['reopened'])
        assert br.same_bits(staged['x0_next'], want['x0_next'])
        for k in range(K):
            sr.compare_tree(ref.tree(k), ds.tree(k), what=(name, case, step, 'restatement', k))
        if step == 0:
            if case == 'states':
                assert list(got['cover'][:4]) == [0, 0, 0, 0] and got['cover'][4] > 0
            else:
                assert np.all(got['cover'] > 0)
            assert with_rows or got['reopened'].sum() > 0
    # the next states are in place: a round stages them
    B = ref.select(1, 0., True)
    assert ds.select(1, 0., True) == B
    if B:
        sr.compare_dicts(ref.batch, ds.batch(), what=(name, case, 'the round after'))


def _one_step(ds, d, specs, node_cap, seed, rounds=None):
    rng = np.random.default_rng(seed)
    covers, u0b = ar.make_covers(d, specs, rng, node_cap)
    x0s = rng.uniform(-1., 1., (len(specs), d['nx']))
    ref = ar.Search(d, len(specs), node_cap, ds.row_cap)
    ref.begin(x0s, [(f, l, None, None) for f, l in covers])
    _begin(ds, d, x0s, covers, None)
    if rounds is None:
        ar.run_step(ref, d, specs, u0b, rng, follow=_follow(ds))
    else:
        for _ in range(rounds):
            B = ref.select(1, 0., True)
            rec = ar.records_for(ref, d, specs, u0b, rng)
            _follow(ds)(1, B, rec)
            ref.put_records(rec)
            ref.consume(0.)
    return ref


def test_refusals_leave_the_trees_and_the_pool_as_they_were():
    from helpers import random_mld, _NoBackend
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    from warm_start_hmpc_amd.search import DeviceSearch, SearchTooBig
    ctrl, qp, d, _ = _ready('random_mld_t5')
    lib = qp.lib
    # how many leaves the trees keep
    probe = DeviceSearch(ctrl, 5, node_cap=420, row_cap=2048)
    _one_step(probe, d, SIZES, 420, 3)
    B = int(probe.advance()['cover'].sum())
    assert B > 64
    # a pool of exactly that many rows takes them, one row less refuses
    full = DeviceSearch(ctrl, 5, node_cap=420, row_cap=B)
    _one_step(full, d, SIZES, 420, 3)
    assert int(full.advance()['cover'].sum()) == B and full.batch(device=True)['row0'] == B
    short = DeviceSearch(ctrl, 5, node_cap=420, row_cap=B - 1)
    _one_step(short, d, SIZES, 420, 3)
    snap = _snapshot(short)
    with pytest.raises(SearchTooBig, match='row_cap'):
        short.advance()
    _unchanged(short, snap, 'row_cap short by one')
    # a running tree; a staged round
    ds = DeviceSearch(ctrl, 5, node_cap=160, row_cap=2048)
    ref = _one_step(ds, d, STATES, 160, 4, rounds=1)
    assert ref.trees[4].state == 0 and ref.trees[4].inc >= 0
    snap = _snapshot(ds)
    assert lib.hmpc_search_advance(ds._s, None, None, None, None, None) == -1 and b'still running' in lib.hmpc_last_error()
    _unchanged(ds, snap, 'a running tree')
    assert ds.select(1, 0., True) > 0
    assert lib.hmpc_search_advance(ds._s, None, None, None, None, None) == -1 and b'staged' in lib.hmpc_last_error()
    _unchanged(ds, snap, 'a staged round')
    # no step has begun; the maps are not set (a handle of its own)
    fresh = DeviceSearch(ctrl, 2, node_cap=8, row_cap=8)
    assert lib.hmpc_search_advance(fresh._s, None, None, None, None, None) == -1 and b'no step has begun' in lib.hmpc_last_error()
    mld, objective, _ = random_mld(nx=6, nuc=2, nub=3, seed=3)
    bare = HybridModelPredictiveController(mld, 5, objective, None, backend=_NoBackend())
    old = os.environ.get('HMPC_JIT')
    os.environ['HMPC_JIT'] = '0'
    try:
        bare.qp = HipBatchedQP(bare.problem_data())
    finally:
        if old is None:
            del os.environ['HMPC_JIT']
        else:
            os.environ['HMPC_JIT'] = old
    nomaps = DeviceSearch(bare, 2, node_cap=8, row_cap=8)
    nomaps.begin(np.zeros((2, d['nx'])))
    snap = _snapshot(nomaps)
    assert lib.hmpc_search_advance(nomaps._s, None, None, None, None, None) == -1 and b'hmpc_set_shift_maps' in lib.hmpc_last_error()
    _unchanged(nomaps, snap, 'maps not set')


def _host_walk(ds, bm, x0s, steps, errors, width, handdown):
    """DeviceSearch.closed_loop's host path, step by step, ending with the begin of the step after the last."""
    from warm_start_hmpc_amd.batched import NodeArrays
    K = ds.K
    xs, ws = np.array(x0s), None
    nothing = NodeArrays(np.zeros((0, ds.nfix), np.int8), np.zeros(0), np.zeros((0, ds.n_dual)), np.zeros(0), np.zeros(0, bool))
    costs = np.full((K, steps), np.nan)
    for t in range(steps):
        res = ds.feedforward_many(xs, ws, width, 0., handdown)
        go = [k for k in range(K) if np.isfinite(res[k]['objective'])]
        new = bm.construct_warm_start_many([res[k]['leaves'] for k in go], xs[go], np.array([np.concatenate((res[k]['uc'][0], res[k]['ub'][0])) for k in go]), errors[go, t])
        ws = [nothing] * K
        for k, w in zip(go, new):
            ws[k], costs[k, t] = w, res[k]['objective']
            xs[k] = res[k]['x'][1] + errors[k, t]
    ds.begin(xs, ws)
    return costs, xs


@pytest.mark.parametrize('handdown', [False, True])
def test_resident_closed_loop_is_the_host_path_to_the_bit(handdown):
    from helpers import load_fixture
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, qp, d, bm = _ready('cart_pole_t20')
    K, steps = 4, 3
    errors = load_fixture('reference_closed_loop')['errors_0003'][:K, :steps]
    x0s = np.array([X0, X0, X0, INFEASIBLE])
    make = lambda: DeviceSearch(ctrl, K, node_cap=1024, row_cap=4096)
    rs, hs = make(), make()
    res = rs.closed_loop(x0s, steps, errors, frontier_width=8, handdown=handdown, resident=True)
    host = hs.closed_loop(x0s, steps, errors, frontier_width=8, handdown=handdown)
    print('handdown %d: costs %s\nnodes %s\nlen_ws %s\nreopened %s' % (handdown, res['costs'], res['nodes_ws'], res['len_ws'], res['reopened']))
    assert br.same_bits(res['costs'], host['costs']) and np.isnan(res['costs'][3]).all() and np.isfinite(res['costs'][:3]).all()
    for key in ('nodes_ws', 'len_ws', 'reopened'):
        assert np.array_equal(res[key], host[key]), key
    assert res['steps'] == host['steps'] == 3 * steps
    assert res['len_ws'][:3].min() > 0 and res['nodes_ws'][:3].min() > 0
    # after the last step: the host path's next begin against the resident search as its last advance left it
    ms = make()
    costs, xs = _host_walk(ms, bm, x0s, steps, errors, 8, handdown)
    assert br.same_bits(costs, res['costs'])
    row0 = ms.batch(device=True)['row0']
    assert rs.batch(device=True)['row0'] == row0 == res['len_ws'][:, -1].sum()
    for k in range(K):
        t = ms.tree(k)
        assert t['n'] == res['len_ws'][k, -1]
        sr.compare_tree({key: v[:t['n']] if key in sr.TREE_ARRAYS else v for key, v in t.items()}, rs.tree(k), what=('tree', k))
    a, b = ms.rows(0, row0), rs.rows(0, row0)
    assert br.same_bits(a['dual'], b['dual']) and br.same_bits(a['dual_obj'], b['dual_obj'])
    # ... and the next states: the round both stage
    assert ms.select(8, 0., handdown) == rs.select(8, 0., handdown) > 0
    sr.compare_dicts(ms.batch(), rs.batch(), what='the round after')
