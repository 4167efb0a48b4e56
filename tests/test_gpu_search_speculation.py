"""Speculation of the device-resident search on the device (hmpc_search_set_speculation; the blocks, offsets, stage and consume
kernels of csrc/hmpc_search.hip), held to the numpy restatement of tests/speculation_reference.py -- integers exactly, floats bit for
bit -- on synthetic rounds, and to itself at depth 0 on whole searches: with hand-down off a search at any depth is the search of
depth 0 in everything but pool row numbers, in fewer launches; against the fleet's speculation; with hand-down on to the solver's
tolerance, every consumed record certified; three resident closed-loop steps."""
import numpy as np
import pytest

import branch_reference as br
import search_reference as sr
import speculation_reference as sp
from test_gpu_branch import _backend
from test_gpu_search import SCAN_CHUNK, X0, INFEASIBLE, _cover_arrays

pytestmark = pytest.mark.gpu
BATCH_KEYS = ('x0', 'fix', 'warm', 'tree', 'node', 'row0')


def _search(name, K, node_cap, row_cap, spec):
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, qp, d = _backend(name)
    return DeviceSearch(ctrl, K, node_cap=node_cap, row_cap=row_cap, speculation=spec), d


def _round(ds, ref, d, width, tol, handdown, rng, what):
    """One synthetic round on both; returns (rows, picks)."""
    B = ref.select(width, tol, handdown)
    assert ds.select(width, tol, handdown) == B and ds._P == ref.P, (what, B, ds._P, ref.P)
    if ref.P == 0:
        return 0, 0
    P = ref.P
    if B:
        sr.compare_dicts({k: ref.batch[k] for k in BATCH_KEYS}, ds.batch(), what=(what, 'batch'))
        rec = sr.synthetic_records(d, ref.batch['fix'], rng)
        sp.scaled(0, ref.batch, rec)
        ref.put_records(rec)
        ds.put_records(rec)
    ref.consume(tol)
    ds.consume(tol)
    return B, P


def _same_state(ds, ref, what, trees):
    sr.compare_dicts(ref.results(), ds.results(), what=(what, 'results'))
    for k in trees:
        sp.compare_tree(ref.tree(k), ds.tree(k), what=(what, 'tree', k))
    assert ds.counters() == {k: int(v) for k, v in ref.count.items()}, (what, ds.counters(), ref.count)


@pytest.mark.parametrize('name,K,width,spec', [('random_mld_t5', 1, 1, 1), ('random_mld_t5', 1, 8, 2), ('random_mld_t5', 1, 8, 4),
                                               ('random_mld_t5', 5, 8, 1), ('random_mld_t5', 5, 3, 2), ('random_mld_t5', 5, 8, 4),
                                               ('cart_pole_t16', 7, 64, 1), ('random_mld_t5', SCAN_CHUNK + 1, 4, 1)])
def test_synthetic_rounds_match_the_restatement(name, K, width, spec):
    # trees of 1, 63, 64, 65 leaves (and a few of 5) whose leaves sit at pos = nfix, nfix - 1, nfix - 2 and shallower: blocks of
    # 1, 3, 7 ... rows side by side; K = 1025: the scan's carry beyond 1024 trees carries emitted rows, not picks; width 64 of the
    # cart-pole: a tree emits more rows than a wavefront has lanes
    rng = np.random.default_rng(1000 * spec + K + width)
    sizes = [(1, 63, 64, 65, 5)[(k + (1 if K == 1 else 0)) % 5] for k in range(K)]
    rounds, cap = 4, 65 + 4 * 2 * width + 2
    rows = sum(sizes) + rounds * K * min(width, 65) * (2 ** (spec + 1) - 1)
    ds, d = _search(name, K, cap, rows, spec)
    covers = []
    for n in sizes:
        f, l = sp.cover(d, n, rng)
        covers.append((f, l, rng.uniform(0., 1., (n, d['n_dual'])), rng.uniform(0., 1., n)))
    ref = sp.Search(d, K, cap, rows, spec=spec)
    x0s = rng.uniform(-1., 1., (K, d['nx']))
    ref.begin(x0s, covers)
    ds.begin(x0s, _cover_arrays(covers))
    watch = list(range(min(K, 10))) + [K - 1]
    _same_state(ds, ref, (name, K, 'begin'), watch)
    seen = []
    for q in range(rounds):
        seen.append(_round(ds, ref, d, width, 0., q % 2 == 0, rng, (name, K, width, spec, q)))
        _same_state(ds, ref, (name, K, width, spec, 'round', q), watch[:3] + [K - 1])
        if seen[-1][1] == 0:
            break
    _same_state(ds, ref, (name, K, width, spec), watch)
    sr.compare_dicts(ref.leaves(), ds.leaves_flat(), what=(name, K, width, spec, 'leaves'))
    assert seen[0][0] > seen[0][1] > 0 and ref.count['served'] > 0              # descendants rode along; waiting records were used
    if K > SCAN_CHUNK:
        assert ref.results()['solves'][K - 1] > 0 and ref.tree(K - 1)['row'].max() > ref.tree(0)['row'].max()   # the tree behind the carry


def test_a_round_writes_its_rows_and_the_weak_dual_objectives_and_nothing_else():
    # every row of the pool is a guard before the rounds; the second round consumes waiting records (one of them WEAK at least)
    ds, d = _search('random_mld_t5', 3, 40, 400, 2)
    rng = np.random.default_rng(5)
    covers = []
    for n in (5, 9, 4):
        f, l = sp.cover(d, n, rng)
        covers.append((f, l, rng.uniform(0., 1., (n, d['n_dual'])), rng.uniform(0., 1., n)))
    ref = sp.Search(d, 3, 40, 400, spec=2)
    x0s = rng.uniform(-1., 1., (3, d['nx']))
    ref.begin(x0s, covers)
    ds.begin(x0s, _cover_arrays(covers))
    guard = dict(obj=np.full(400, -7.), dual_obj=np.full(400, -7.), status=np.full(400, -7, np.int32), iters=np.full(400, -7, np.int32),
                 primal=np.full((400, d['n_primal']), -7.), dual=np.full((400, d['n_dual']), -7.))
    ds.rows(0, 400, guard)                                                      # (the covers' 18 rows included: nothing reads them here)
    first = ref.row0
    sizes = [_round(ds, ref, d, 4, 0., True, rng, ('guards', q)) for q in range(3)]
    assert first == 18 and sizes[0][0] > sizes[0][1] and ref.count['served'] > 0
    pool = ds.rows(0, 400)
    for k in sr.RECORD_KEYS:
        want = guard[k].copy()
        want[first:ref.row0] = ref.pool[k][first:ref.row0]
        assert br.same_bits(want, pool[k]), k
    assert np.isneginf(pool['dual_obj']).any() and ref.row0 < 399


def test_a_round_beyond_the_pool_is_refused_with_nothing_changed_and_the_depth_is_refused_while_a_round_is_staged():
    from warm_start_hmpc_amd.search import SearchTooBig
    ds, d = _search('random_mld_t5', 2, 16, 8 + 6 * 7 - 1, 2)                   # the covers' 8 rows, and one row less than 2 x 3 blocks of 7
    rng = np.random.default_rng(2)
    covers = []
    for k in range(2):
        f, l = sp.cover(d, 4, rng)
        f[:, -3:] = -1                                                          # (every leaf has three free binaries: blocks of 7 rows)
        covers.append((f, l, rng.uniform(0., 1., (4, d['n_dual'])), rng.uniform(0., 1., 4)))
    x0s = np.zeros((2, d['nx']))
    ds.begin(x0s, _cover_arrays(covers))
    before = [ds.tree(k) for k in range(2)]
    with pytest.raises(SearchTooBig, match='row_cap'):
        ds.select(3, 0., True)
    for k in range(2):
        after = ds.tree(k)
        for key in before[k]:
            assert br.same_bits(np.asarray(before[k][key]), np.asarray(after[key])), (k, key)
    ds.set_speculation(1)                                                       # (nothing is staged after a refusal)
    assert ds.select(3, 0., True) == 2 * 3 * 3 and ds._P == 6
    with pytest.raises(ValueError, match='staged'):
        ds.set_speculation(2)
    for depth in (-1, 5):
        with pytest.raises(ValueError, match='0 .. 4'):
            ds.set_speculation(depth)
    assert ds.speculation == 1


# ---- whole searches ---------------------------------------------------------------------------------------------------------------
def _quarter_grid(qp, d):
    """A quarter of the nodes the handle keeps resident: up to there every launch runs four waves per node, and records do not
    depend on the size of their batch (read from the launch info after one launch larger than the device)."""
    fix = np.full((4096, d['nfix']), -1, np.int8)
    qp.solve_batch(X0, fix, want_primal=False, want_dual=False)
    grid = qp.launch_info()[0]
    assert 0 < grid < 4096
    return grid // 4


def _whole(ds, x0s, width, handdown, most):
    """A whole search round by round, every launch of at most `most` rows; returns what it left."""
    ds.begin(x0s)
    while True:
        rounds, B = ds.run(width, 0., handdown, max_rounds=1)
        if rounds == 0:
            break
        assert B <= most, (B, most)
    row0 = ds.batch()['row0']
    return dict(results=ds.results(), leaves=ds.leaves_flat(), trees=[ds.tree(k) for k in range(ds.K)], pool=ds.rows(0, row0), counters=ds.counters())


@pytest.mark.parametrize('width', [1, 8])
def test_cart_pole_searches_at_depths_one_and_two_are_the_search_of_depth_zero(width):
    from warm_start_hmpc_amd.fleet import FleetMPC
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, qp, d = _backend('cart_pole_t20')
    most = _quarter_grid(qp, d)
    x0s = np.array([X0, X0 * .5, INFEASIBLE])
    ds = DeviceSearch(ctrl, 3, node_cap=1024, row_cap=16384)
    base = _whole(ds, x0s, width, False, most)
    assert np.array_equal(base['results']['state'], [sr.DONE | sr.INCUMBENT, sr.DONE | sr.INCUMBENT, sr.DONE]) and base['results']['solves'][0] > 20
    assert base['counters']['launches'] == base['counters']['rounds'] and base['counters']['served'] == 0
    for spec in (1, 2):
        ds.set_speculation(spec)
        got = _whole(ds, x0s, width, False, most)
        print('width %d depth %d: %s against %s at depth 0' % (width, spec, got['counters'], base['counters']))
        sr.compare_dicts(base['results'], got['results'], what=(width, spec, 'results'))
        sr.compare_dicts(base['leaves'], got['leaves'], what=(width, spec, 'leaves'))
        for k in range(3):
            sp.compare_modulo_rows(base['trees'][k], got['trees'][k], base['pool'], got['pool'], what=(width, spec, 'tree', k))
        assert got['counters']['launches'] < base['counters']['launches'] and got['counters']['rounds'] == base['counters']['rounds']
        assert got['counters']['rows'] >= got['results']['solves'].sum() and got['counters']['served'] > 0
        if width == 8:                                                          # the fleet's speculation at the same depth: the same searches
            fl = FleetMPC(ctrl, 3, handdown=False).solve(x0s, 8, speculation=spec)
            assert br.same_bits(fl['cost'], got['results']['cost']) and np.array_equal(fl['solves'], got['results']['solves'])
    ds.set_speculation(0)


def _consumed(tree):
    """(identifier, pool row) of every record the tree consumed: a row is carried by the node it was solved for and by that node's
    children until they are solved themselves -- the node is the one with the fewest fixed binaries."""
    n = tree['n']
    out = {}
    for i in range(n):
        r = int(tree['row'][i])
        if r >= 0 and (r not in out or sp.pos_of(tree['fix'][i]) < sp.pos_of(tree['fix'][out[r]])):
            out[r] = i
    return sorted((r, i) for r, i in out.items())


def test_with_hand_down_depth_two_finds_the_costs_of_depth_zero_and_consumes_certified_records():
    from certificates import assert_certified, record_from_device
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, qp, d = _backend('cart_pole_t20')
    x0s = np.array([X0, X0 * .5, INFEASIBLE])
    ds = DeviceSearch(ctrl, 3, node_cap=1024, row_cap=16384)
    base = _whole(ds, x0s, 8, True, 4096)
    ds.set_speculation(2)
    got = _whole(ds, x0s, 8, True, 4096)
    np.testing.assert_allclose(got['results']['cost'], base['results']['cost'], rtol=1e-9, atol=1e-12)
    assert np.array_equal(got['results']['state'], base['results']['state']) and got['counters']['launches'] < base['counters']['launches']
    assert (got['pool']['iters'] & br.HANDED_BIT).any()                        # (records were still handed down, to the blocks' first rows)
    for k in range(3):
        pairs = _consumed(got['trees'][k])
        rows, nodes = [r for r, _ in pairs], [i for _, i in pairs]
        assert len(rows) == got['results']['solves'][k]
        rec = record_from_device(*[got['pool'][key][rows] for key in ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual')])
        assert_certified(ctrl, x0s[k], got['trees'][k]['fix'][nodes], rec, what='depth 2, hand-down, tree %d' % k)


def test_three_resident_closed_loop_steps_at_depth_one_are_those_of_depth_zero():
    from helpers import load_fixture
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, qp, d = _backend('cart_pole_t20')
    K, steps = 4, 3
    errors = load_fixture('reference_closed_loop')['errors_0003'][:K, :steps]
    plain = DeviceSearch(ctrl, K, node_cap=1024, row_cap=8192).closed_loop(X0, steps, errors, frontier_width=8, handdown=False, resident=True)
    ds = DeviceSearch(ctrl, K, node_cap=1024, row_cap=8192, speculation=1)
    spec = ds.closed_loop(X0, steps, errors, frontier_width=8, handdown=False, resident=True)
    assert br.same_bits(spec['costs'], plain['costs']) and np.isfinite(plain['costs']).all()
    for key in ('len_ws', 'reopened', 'nodes_ws'):
        assert np.array_equal(spec[key], plain[key]), key
    assert spec['steps'] == plain['steps'] == K * steps and ds.counters()['served'] > 0
