"""hmpc_branch_batch / hmpc_branch_batch_device on the device (csrc/hmpc_branch.hip), held to the numpy restatement of
tests/branch_reference.py -- integers exactly, floats bit for bit, the comparisons of the CPU form in tests/test_branch_host.py --;
the solve -> branch -> solve chain on one stream; the fleet with and without the digest of a round."""
import numpy as np
import pytest

import branch_reference as br

pytestmark = pytest.mark.gpu
SCAN_CHUNK = 1024          # BRANCH_SCAN_CHUNK of csrc/hmpc_branch.hip: nodes per pass of the offsets kernel
_BACKENDS = {}


def _backend(name):
    """(HipBatchedQP, dims) per problem, one handle each.  nfix = 80: two words of bits, the second partial; 15: less than a wave;
    64: exactly one word.  Only the first is ever solved on: the others branch synthetic records and need no compiled kernel."""
    import os
    from helpers import make_controller, random_mld, _NoBackend
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    if name not in _BACKENDS:
        if name == 'cart_pole_t20':
            ctrl = make_controller('cart_pole_with_walls', T=20, backend='hip')
        else:
            if name == 'random_mld_t5':
                mld, objective, _ = random_mld(nx=6, nuc=2, nub=3, seed=3)
                ctrl = HybridModelPredictiveController(mld, 5, objective, None, backend=_NoBackend())
            else:
                assert name == 'cart_pole_t16'
                ctrl = make_controller('cart_pole_with_walls', T=16, backend=_NoBackend())
            old = os.environ.get('HMPC_JIT')
            os.environ['HMPC_JIT'] = '0'                                       # (the shipped kernels would serve: nothing is compiled)
            try:
                ctrl.qp = HipBatchedQP(ctrl.problem_data())
            finally:
                if old is None:
                    del os.environ['HMPC_JIT']
                else:
                    os.environ['HMPC_JIT'] = old
        d = br.dims_of(ctrl.problem_data())
        assert (d['n_primal'], d['n_dual']) == (ctrl.qp.n_primal, ctrl.qp.n_dual)
        _BACKENDS[name] = (ctrl, ctrl.qp, d)
    return _BACKENDS[name]


NFIX = {'cart_pole_t20': 80, 'random_mld_t5': 15, 'cart_pole_t16': 64}
GUARD = -7


def _device_call(qp, d, fix, rec, cutoff=None, warm_base=0, mark_weak=False, want=br.OUTPUTS):
    """branch_batch_device with one guard row behind every output (and the guard value in every row: the children beyond
    n_children must keep it).  Returns the outputs as ``reference`` returns them, dual_obj included."""
    import torch
    dev = torch.device('cuda', 0)
    B, nfix = len(fix), d['nfix']
    t = lambda a, dtype: torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)
    r = dict(obj=t(rec['obj'], torch.float64), dual_obj=t(rec['dual_obj'], torch.float64), status=t(rec['status'], torch.int32),
             iters=t(rec['iters'], torch.int32), primal=t(rec['primal'], torch.float64), dual=t(rec['dual'], torch.float64))
    shapes = dict(obj=((B,), torch.float64), word=((B,), torch.int32), pos=((B,), torch.int32), child_lb2=((B, 2), torch.float64),
                  bits=((B, d['words']), torch.int64), child_offset=((B,), torch.int32), n_children=((1,), torch.int32),
                  child_fix=((2 * B, nfix), torch.int8), child_lb=((2 * B,), torch.float64), child_parent=((2 * B,), torch.int32),
                  child_warm=((2 * B,), torch.int32))
    full = {k: torch.full((s[0] + 1,) + s[1:], GUARD, dtype=dtype, device=dev) for k, (s, dtype) in shapes.items()}
    out = {k: full[k][:shapes[k][0][0]] for k in want}
    qp.branch_batch_device(t(fix, torch.int8), r, out, cutoff=t(cutoff, torch.float64) if cutoff is not None else None,
                           warm_base=warm_base, mark_weak=mark_weak)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in full.items()}
    for k, v in got.items():
        assert np.all(v[-1] == GUARD), ('guard row', k)
        if k not in want:
            assert np.all(v == GUARD), ('not asked for, yet written', k)
    res = {k: got[k][:-1] for k in want}
    if 'n_children' in res:
        n = res['n_children'] = int(res['n_children'][0])
        for k in br.CHILDREN:
            if k in res:
                assert np.all(res[k][n:] == GUARD), ('rows beyond n_children', k)
                res[k] = res[k][:n]
    res['dual_obj'] = r['dual_obj'].cpu().numpy()
    for k in ('obj', 'status', 'iters', 'primal', 'dual'):                       # nothing else of the records is written
        assert br.same_bits(r[k].cpu().numpy(), np.ascontiguousarray(rec[k], dtype=r[k].cpu().numpy().dtype)), k
    return res


def _host_call(qp, fix, rec, cutoff=None, warm_base=0, mark_weak=False, want=None):
    out = qp.branch_batch(fix, rec, cutoff=cutoff, warm_base=warm_base, mark_weak=mark_weak, want=want)
    if not mark_weak:
        out['dual_obj'] = np.asarray(rec['dual_obj'], np.float64)
    return out


def _both(qp, d, fix, rec, what, cutoff=None, warm_base=0, mark_weak=False):
    ref = br.reference(d, fix, rec, cutoff, warm_base, mark_weak=True) if mark_weak else dict(br.reference(d, fix, rec, cutoff, warm_base), dual_obj=np.asarray(rec['dual_obj'], np.float64))
    dev = _device_call(qp, d, fix, rec, cutoff, warm_base, mark_weak)
    br.compare(ref, dev, what=(what, 'device'))
    host = _host_call(qp, fix, rec, cutoff, warm_base, mark_weak)
    br.compare(ref, host, what=(what, 'host'))
    assert set(ref) <= set(dev) and set(ref) <= set(host)
    return ref


@pytest.mark.parametrize('name', list(NFIX))
@pytest.mark.parametrize('B', [1, 63, 65, SCAN_CHUNK + 1])
def test_synthetic_records_on_wave_workgroup_and_scan_chunk_edges(name, B):
    # B = 1, 63, 65: below and across a wave of nodes and a workgroup of four; B = 1025: one node past the 1024 nodes the offsets
    # kernel sums per pass (SCAN_CHUNK), so that the carry between two passes decides the last offset
    ctrl, qp, d = _backend(name)
    assert d['nfix'] == NFIX[name]
    fix, rec = br.synthetic(d, B, seed=B)
    cutoff = br.half_cutoff(rec)
    cutoff[-1] = np.inf                                                        # (the last node branches where its record allows)
    ref = _both(qp, d, fix, rec, (name, B), cutoff=cutoff, warm_base=3, mark_weak=True)
    if B > 16:
        assert 0 < ref['n_children'] < 2 * B and (ref['word'] & br.PRUNED).any() and (ref['bits'] != 0).any()
        weak = (rec['iters'] & br.WEAK_BIT) != 0
        assert weak.any() and np.all(np.isneginf(ref['dual_obj'][weak])) and br.same_bits(ref['dual_obj'][~weak], rec['dual_obj'][~weak])
    if B > SCAN_CHUNK:
        assert ref['child_offset'][SCAN_CHUNK] > 0 and ref['word'][SCAN_CHUNK] & br.BRANCHED                  # children behind the carry


@pytest.mark.parametrize('mode', ['none', 'all', 'alternating'])
@pytest.mark.parametrize('cut', ['null', 'inf'])
def test_none_all_and_every_other_node_branched(mode, cut):
    ctrl, qp, d = _backend('cart_pole_t20')
    fix, rec = br.synthetic(d, 65, seed=11, mode=mode)
    ref = _both(qp, d, fix, rec, mode, cutoff=None if cut == 'null' else np.full(65, np.inf), mark_weak=False)
    assert ref['n_children'] == dict(none=0, all=130, alternating=66)[mode]


def test_real_records_of_a_mixed_depth_frontier():
    from helpers import random_prefix_frontier
    ctrl, qp, d = _backend('cart_pole_t20')
    x0 = np.array([0., 0., .5, 0.])
    fix = np.vstack((np.full((1, 80), -1, np.int8), random_prefix_frontier(20, 4, 47, p_one=0.1)))
    for depth in (1, 2, 5, 17, 64, 79, 80):                                     # the all-zero dive: optimal nodes at every depth, one complete
        fix = np.vstack((fix, np.concatenate((np.zeros(depth, np.int8), np.full(80 - depth, -1, np.int8)))[None]))
    solved = qp.solve_batch(x0, fix)
    rec = br.as_word_records(solved)
    assert (rec['status'] == 0).sum() >= 8 and (rec['status'] == 1).sum() >= 10 and (rec['status'] > 1).sum() == 0
    for cutoff in (None, br.half_cutoff(rec)):
        ref = _both(qp, d, fix, rec, 'real records', cutoff=cutoff, warm_base=5, mark_weak=True)
        assert (ref['word'] & br.BRANCHED).sum() >= 4 and (ref['word'] & br.COMPLETE).sum() >= (cutoff is None) and (ref['word'] & br.INFEASIBLE).sum() >= 10
    # the project's own definition of a child: controller._brancher with branch_in_time
    out = _host_call(qp, fix, rec)
    kids = br.brancher_children(ctrl, fix, solved)
    assert len(kids) >= 8
    for b, (ids, lbs) in kids.items():
        rows = slice(out['child_offset'][b], out['child_offset'][b] + 2)
        assert out['word'][b] & br.BRANCHED and np.array_equal(ids, out['child_fix'][rows]) and br.same_bits(lbs, out['child_lb'][rows]), b


@pytest.mark.parametrize('left_out', br.OUTPUTS)
def test_each_member_may_be_null_and_nothing_else_changes(left_out):
    ctrl, qp, d = _backend('cart_pole_t20')
    fix, rec = br.synthetic(d, 65, seed=5)
    want = tuple(k for k in br.OUTPUTS if k != left_out and not (left_out == 'child_offset' and k in br.CHILDREN))
    ref = br.reference(d, fix, rec, br.half_cutoff(rec), warm_base=9)
    dev = _device_call(qp, d, fix, rec, br.half_cutoff(rec), warm_base=9, want=want)          # (checks that what was left out stays untouched)
    host = _host_call(qp, fix, rec, br.half_cutoff(rec), warm_base=9, want=want)
    for got, rest in ((dev, GUARD), (host, 0)):
        assert set(want) <= set(got) and left_out not in got
        if left_out == 'n_children':                                                           # (nobody could cut the children: rows beyond stay as they were)
            for k in br.CHILDREN:
                assert got[k].shape[0] == 2 * 65 and np.all(got[k][ref['n_children']:] == rest), k
                got[k] = got[k][:ref['n_children']]
        br.compare(ref, got, what=left_out, keys=[k for k in want if k != 'n_children' or 'n_children' in got])


def test_child_arrays_without_offsets_are_refused_and_an_empty_batch_touches_nothing():
    import ctypes
    import torch
    from warm_start_hmpc_amd.qp_backend import _Result, _BranchOut
    ctrl, qp, d = _backend('cart_pole_t20')
    fix, rec = br.synthetic(d, 4, seed=1)
    with pytest.raises(RuntimeError, match='child_offset'):
        qp.branch_batch(fix, rec, want=('child_fix', 'n_children'))
    empty = _device_call(qp, d, fix[:0], {k: v[:0] for k, v in rec.items()})                  # B == 0 through the binding: every guard untouched
    assert empty['n_children'] == GUARD
    keep = {k: np.ascontiguousarray(v) for k, v in rec.items()}
    r = _Result(**{k: v.ctypes.data for k, v in keep.items()})
    n = np.full(1, GUARD, np.int32)
    o = _BranchOut(n_children=n.ctypes.data)
    assert qp.lib.hmpc_branch_batch(qp.handle, fix.ctypes.data, 0, ctypes.byref(r), None, 0, 0, ctypes.byref(o)) == 0 and n[0] == GUARD
    assert qp.lib.hmpc_branch_batch(qp.handle, fix.ctypes.data, -1, ctypes.byref(r), None, 0, 0, ctypes.byref(o)) == -1
    assert qp.lib.hmpc_branch_batch(qp.handle, fix.ctypes.data, 4, ctypes.byref(r), None, 0, 0, ctypes.byref(o)) == 0 and n[0] == br.reference(d, fix, rec)['n_children']
    torch.cuda.synchronize()


def test_solve_branch_solve_three_levels_on_one_stream():
    """root -> children -> grandchildren -> great-grandchildren: solve_batch_device, branch_batch_device, solve_batch_device on
    child_fix with child_warm as the hand-down index, on ONE stream; between two launches only n_children comes to the host."""
    import torch
    from helpers import make_controller, record_close
    from certificates import assert_certified, record_from_device
    hip = make_controller('cart_pole_with_walls', T=10, backend='hip')
    qp, dev = hip.qp, torch.device('cuda', 0)
    nfix = qp.nfix
    x0 = np.array([0., 0., .5, 0.])
    d_x0 = torch.tensor(x0, device=dev)
    stream = torch.cuda.Stream(device=dev)

    def records(B):
        return dict(obj=torch.empty(B, dtype=torch.float64, device=dev), dual_obj=torch.empty(B, dtype=torch.float64, device=dev),
                    status=torch.empty(B, dtype=torch.int32, device=dev), iters=torch.empty(B, dtype=torch.int32, device=dev),
                    primal=torch.empty((B, qp.n_primal), dtype=torch.float64, device=dev), dual=torch.empty((B, qp.n_dual), dtype=torch.float64, device=dev))

    warm, levels = None, []
    with torch.cuda.stream(stream):
        fix = torch.full((1, nfix), -1, dtype=torch.int8, device=dev)            # (filled on the stream that reads it)
        for level in range(4):
            B = fix.shape[0]
            rec = records(B)
            qp.solve_batch_device(d_x0, fix, rec, stream=stream.cuda_stream, warm=warm)
            levels.append((fix, rec, warm))
            if level == 3:
                break
            out = dict(child_offset=torch.empty(B, dtype=torch.int32, device=dev), n_children=torch.empty(1, dtype=torch.int32, device=dev),
                       child_fix=torch.empty((2 * B, nfix), dtype=torch.int8, device=dev), child_lb=torch.empty(2 * B, dtype=torch.float64, device=dev),
                       child_warm=torch.empty(2 * B, dtype=torch.int32, device=dev))
            qp.branch_batch_device(fix, rec, out, warm_base=0, stream=stream.cuda_stream)
            n = int(out['n_children'].cpu()[0])                                  # the one value read back: it sizes the next launch
            assert 0 < n <= 2 * B and n % 2 == 0, (level, n, B)
            fix = out['child_fix'][:n]
            warm = (rec['primal'], rec['dual'], out['child_warm'][:n].contiguous())
    stream.synchronize()
    keys = ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual')
    fix3, rec3, warm3 = levels[3]
    h_fix, index = fix3.cpu().numpy(), warm3[2].cpu().numpy()
    # the last level is what the reference makes of the level before it: ordered, 0-branch first, the rows to hand down
    fix2, rec2 = levels[2][0].cpu().numpy(), {k: levels[2][1][k].cpu().numpy() for k in keys}
    ref = br.reference(br.dims_of(hip.problem_data()), fix2, rec2)
    assert ref['n_children'] == len(h_fix) >= 2 and np.array_equal(ref['child_fix'], h_fix) and np.array_equal(ref['child_warm'], index)
    assert np.all((h_fix >= 0).sum(axis=1) == 3) and np.all(h_fix[:, 3:] == -1)
    got = record_from_device(*[rec3[k].cpu().numpy() for k in keys])
    host = qp.solve_batch(x0, h_fix, warm=(rec2['primal'], rec2['dual'], index))
    print('level 3: %d nodes, statuses %s, %d handed down' % (len(h_fix), got['status'].tolist(), int(((rec3['iters'].cpu().numpy() >> 18) & 1).sum())))
    assert np.array_equal(got['status'], host['status'])
    record_close(got, host, tol=1e-5)
    assert_certified(hip, x0, h_fix, got, what='solve -> branch -> solve, level 3')


@pytest.mark.parametrize('width', [1, 8])
@pytest.mark.parametrize('speculation', [0, 2, -1])
def test_fleet_with_the_digest_walks_the_same_walk(width, speculation):
    from helpers import make_controller, load_fixture
    from warm_start_hmpc_amd.fleet import FleetMPC
    if 'fleet' not in _BACKENDS:
        _BACKENDS['fleet'] = make_controller('cart_pole_with_walls', backend='hip')
    ctrl = _BACKENDS['fleet']
    K, steps = 8, 4
    errors = load_fixture('reference_closed_loop')['errors_0003'][:K, :steps]
    off, on = FleetMPC(ctrl, K, digest=False), FleetMPC(ctrl, K, digest=True)
    assert not off.digest and on.digest
    xs = np.repeat(np.array([[0., 0., 1., 0.]]), K, axis=0)
    for t in range(steps):
        a, b = off.solve(xs, width, speculation=speculation), on.solve(xs, width, speculation=speculation)
        for k in ('cost', 'u0', 'x1', 'solves', 'leaves'):
            assert br.same_bits(a[k], b[k]), (t, k, a[k], b[k])
        (ca, ra), (cb, rb) = off.shift(errors[:, t]), on.shift(errors[:, t])
        assert np.array_equal(ca, cb) and np.array_equal(ra, rb), (t, ca, cb, ra, rb)
        assert np.all(np.isfinite(a['cost'])) and np.all(ca > 0)
        xs = a['x1'] + errors[:, t]
    sa, sb = off.stats(), on.stats()
    assert {k: v for k, v in sa.items() if k != 'seconds'} == {k: v for k, v in sb.items() if k != 'seconds'}, (sa, sb)
    assert sa['rounds'] > steps and sa['launched'] >= K * steps
