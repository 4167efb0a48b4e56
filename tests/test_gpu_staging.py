"""The host-pointer entries of one handle, one after the other, each held to the device-pointer entry of its family on torch
tensors with the same inputs -- integers exactly, floats bit for bit.  The host-pointer entries share the handle's staging blocks
(solve, certify, branch) or grow their own (shift, search), with offsets of the current batch inside a capacity left by an earlier
one: a stale capacity, or a block shared between two families, is what this sequence would show.  Then one device search with a
cover through begin / run / results / leaves against the restatement of tests/search_reference.py.

Every solve is launched twice through the device-pointer entry, into outputs that hold two different quiet-NaN payloads
(integers: two non-zero words): an entry whose bits equal its fill was not written, and there must be none, in any array; the two
launches and the host-pointer entry must agree to the bit in every array.  That includes the solve with a hand-down (step 6) and
the dual rows of its handed nodes.  Those rows used to differ from launch to launch -- first seen here, with fills of +0. and -0.,
as "7 entries of 2 of the 22 handed rows left unwritten"; every entry was written, which launch held zeros for the bounds'
multipliers of the binaries a verified hand-down fixes changed (tests/test_gpu_handdown_records.py has the cause and holds the
hand-down on every kernel family; here it is held in the company of the other entries of one handle).  A wrong row or offset of the
gathered hand-down changes the active set a handed node tries: it shows in iters, in the handed flag and in the records, all
compared to the bit."""
import numpy as np
import pytest

import branch_reference as br
import search_reference as sr
from helpers import make_controller, random_prefix_frontier

pytestmark = pytest.mark.gpu
X0 = np.array([0., 0., .5, 0.])
T = 10
RECORD = ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual')


FILLS = ((0x7ff80000dead0001, 0x5a5a5a5a), (0x7ff80000beef0002, 0x3c3c3c3c))     # (neither NaN is the 0x7ff8000000000000 the kernel writes for the primal row of an infeasible node)


def _fill(shape, integer, which):
    return np.full(shape, FILLS[which][1], np.uint32).view(np.int32) if integer else np.full(shape, FILLS[which][0], np.uint64).view(np.float64)


def _tensors(B, qp, primal=True, dual=True, fill=0):
    """Outputs of a batch of B nodes that hold fill ``fill`` of FILLS, uploaded as bit patterns."""
    shapes = dict(obj=(B,), dual_obj=(B,), status=(B,), iters=(B,), primal=(B, qp.n_primal) if primal else None, dual=(B, qp.n_dual) if dual else None)
    return {k: None if s is None else _to(_fill(s, k in ('status', 'iters'), fill)) for k, s in shapes.items()}


def _to(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', 0))


def _device_solve(qp, x0, fix, primal=True, dual=True, warm=None, fill=0):
    """Records of the device-pointer solve, ``iters`` the word of the C ABI; the outputs hold fill ``fill`` of FILLS before the launch."""
    import torch
    out = _tensors(len(fix), qp, primal, dual, fill)
    qp.solve_batch_device(_to(x0), _to(fix), out, warm=None if warm is None else tuple(_to(a) for a in warm))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _bits_differ(a, b):
    """Per entry: not the same bits (NaN payloads and signed zeros included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    return (a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,))).any(axis=-1)


def _same_solve(qp, x0, fix, what, primal=True, dual=True, warm=None):
    """Host-pointer against device-pointer solve, and two launches of the latter into differently filled outputs, bit for bit.
    Returns (records of the device entry, {array: mask of the entries a launch left unwritten}): the caller asserts there is none."""
    host = qp.solve_batch(x0, fix, want_primal=primal, want_dual=dual, warm=warm)
    dev = _device_solve(qp, x0, fix, primal, dual, warm, fill=0)
    other = _device_solve(qp, x0, fix, primal, dual, warm, fill=1)
    assert (host['primal'] is None) == (not primal) and (host['dual'] is None) == (not dual)
    host = dict(host, iters=br.iters_word(host))
    unwritten = {k: ~_bits_differ(dev[k], _fill(dev[k].shape, k in ('status', 'iters'), 0)) | ~_bits_differ(other[k], _fill(other[k].shape, k in ('status', 'iters'), 1))
                 for k in dev}
    for k in dev:
        for name, rec in (('host-pointer entry', host), ('second launch', other)):
            bad = _bits_differ(np.ascontiguousarray(rec[k]), dev[k])
            rows = np.flatnonzero(bad.reshape(len(fix), -1).any(axis=1))
            with np.errstate(invalid='ignore'):
                gap = np.abs(np.asarray(rec[k], np.float64) - dev[k])[bad]
            figures = '%s, %s: %d entries of rows %s of the %s differ from the first launch, by at most %.3e' % (
                what, k, int(bad.sum()), rows.tolist(), name, float(np.nanmax(gap)) if np.isfinite(gap).any() else 0.)
            assert not bad.any(), figures
    assert (dev['status'] <= 1).all(), (what, dev['status'])
    return dev, unwritten


def _same_certificates(qp, x0, fix, rec, what):
    import torch
    from warm_start_hmpc_amd.qp_backend import CERT_COLUMNS, CERT_CLASSES, CERT_FAILED
    B = len(fix)
    flagged = dict(rec, iters=rec['iters'] & 0xFFFF, polished=(rec['iters'] >> 16) & 1, weak=(rec['iters'] >> 17) & 1)
    host = qp.certify_batch(x0, fix, flagged)
    res = torch.full((B, len(CERT_COLUMNS)), -7., dtype=torch.float64, device=torch.device('cuda', 0))
    verdict = torch.full((B,), -7, dtype=torch.int32, device=torch.device('cuda', 0))
    qp.certify_batch_device(_to(x0), _to(fix), {k: _to(rec[k]) for k in RECORD}, res, verdict)
    torch.cuda.synchronize()
    res, verdict = res.cpu().numpy(), verdict.cpu().numpy()
    for c, name in enumerate(CERT_COLUMNS):
        assert br.same_bits(host[name], np.ascontiguousarray(res[:, c])), (what, name)
    assert np.array_equal(host['class'], np.array(CERT_CLASSES, dtype=object)[verdict & 0xFF]), what
    assert np.array_equal(host['failed'], (verdict & CERT_FAILED) != 0) and np.array_equal(host['failed_mask'], (verdict >> 16) & 0xFFFF), what
    assert (host['class'] != 'skipped').all() and np.isfinite(res).any(axis=1).all(), what      # (nothing compared was empty)


def _same_branching(qp, d, fix, rec, what, want=br.OUTPUTS, **kw):
    from test_gpu_branch import _device_call, _host_call
    dev = _device_call(qp, d, fix, rec, want=want, **kw)
    host = _host_call(qp, fix, rec, want=want, **kw)
    assert set(want) <= set(host) and set(host) == set(dev), (what, set(host), set(dev))
    br.compare(dev, host, what=what)
    return host


def test_one_handle_through_every_host_pointer_entry():
    import torch
    ctrl = make_controller('cart_pole_with_walls', T=T, backend='hip')
    qp, d = ctrl.qp, br.dims_of(ctrl.problem_data())
    qp.set_shift_maps(ctrl._update['mu'], ctrl._update['rho'], ctrl.mld.V)
    nub, nfix = d['nub'], d['nfix']
    frontier = random_prefix_frontier(T, nub, 300, p_one=0.1)
    frontier[0, :] = -1
    # 1. a small batch, primal rows only, one shared x0: the blocks are allocated for 64 nodes without records handed down
    assert not any(m.any() for m in _same_solve(qp, X0, frontier[:3], 'solve 3', dual=False)[1].values())
    # 2. certificates of 130 records: the same blocks, grown to an exact fit with another layout
    rec300 = _device_solve(qp, X0, frontier)                                    # (the device-pointer entry stages nothing)
    fix130, rec130 = frontier[:130], {k: v[:130].copy() for k, v in rec300.items()}
    _same_certificates(qp, X0, fix130, rec130, 'certify 130')
    # 3. branching one node for the number of its children alone: four bytes of the copy down
    one = _same_branching(qp, d, fix130[:1], {k: v[:1] for k, v in rec130.items()}, 'branch 1', want=('n_children',))
    assert one['n_children'] == 2
    # 4. branching seven nodes for everything, with a cutoff and weak nodes marked
    rec7 = {k: v[:7].copy() for k, v in rec130.items()}
    cutoff = br.half_cutoff(rec7)
    cutoff[0] = np.inf
    seven = _same_branching(qp, d, fix130[:7], rec7, 'branch 7', cutoff=cutoff, warm_base=3, mark_weak=True)
    assert 0 < seven['n_children'] <= 14 and len(seven['child_fix']) == seven['n_children']
    # 5. the shift of five leaves of two trees: a block of its own
    optimal = np.flatnonzero(rec130['status'] == 0)[:5]
    w = dict(owner=np.array([0, 1, 0, 1, 0], np.int32), x0=np.array([X0, X0 * .8]), u0=np.zeros((2, d['nu'])), e0=np.array([X0 * .01, -X0 * .01]),
             fix=fix130[optimal].copy(), lb=rec130['obj'][optimal].copy(), dual=rec130['dual'][optimal].copy(), dobj=rec130['dual_obj'][optimal].copy())
    w['fix'][:, :nub] = np.array([-1, 0, -1, 0, 1], np.int8)[:, None]           # (free, as applied, free, as applied, against the applied input)
    host = qp.shift_batch(w['owner'], w['x0'], w['u0'], w['e0'], w['fix'], w['lb'], w['dual'], w['dobj'])
    t = {k: _to(v) for k, v in w.items()}
    out = dict(fix=torch.zeros_like(t['fix']), lb=torch.zeros_like(t['lb']), dual=torch.zeros_like(t['dual']), dual_obj=torch.zeros_like(t['dobj']),
               flags=torch.zeros(5, dtype=torch.uint8, device=t['fix'].device))
    qp.shift_batch_device(t['owner'], t['x0'], t['u0'], t['e0'], t['fix'], t['lb'], t['dual'], t['dobj'], out)
    torch.cuda.synchronize()
    flags = out['flags'].cpu().numpy()
    keep = (flags & 1).astype(bool)
    assert np.array_equal(host['keep'], keep) and np.array_equal(host['reopened'], (flags & 2).astype(bool)) and keep.any(), flags
    for k in ('fix', 'lb', 'dual', 'dual_obj'):                                  # (rows of dropped leaves are undefined)
        assert br.same_bits(host[k][keep], out[k].cpu().numpy()[keep]), ('shift', k)
    # 6. 65 children, a third of them handed their parent's record: past the 64 nodes of the first allocation, now with room for records
    parents = np.flatnonzero((frontier < 0).any(axis=1) & (rec300['status'] == 0))[:65]
    assert len(parents) == 65
    fix65 = frontier[parents].copy()
    fix65[np.arange(65), (fix65 < 0).argmax(axis=1)] = 0
    index = np.where(np.arange(65) % 3 == 0, parents, -1).astype(np.int32)
    handed, unwritten = _same_solve(qp, X0, fix65, 'solve 65 handed', warm=(rec300['primal'], rec300['dual'], index))
    verified = ((handed['iters'] >> 18) & 1) > 0
    assert verified.any() and not (verified & (index < 0)).any()               # (records were handed down, and some verified)
    assert not any(m.any() for m in unwritten.values()), {k: np.flatnonzero(m.reshape(65, -1).any(axis=1)).tolist() for k, m in unwritten.items()}
    # 7. 300 cold nodes: the blocks grow again, and the hand-down region is empty
    assert not any(m.any() for m in _same_solve(qp, X0, frontier, 'solve 300')[1].values())
    # 8. two nodes inside the capacity of 300, both records, an x0 per node
    assert not any(m.any() for m in _same_solve(qp, np.array([X0, X0 * .8]), frontier[5:7], 'solve 2')[1].values())
    # 9. one certificate in the block the solves left behind
    _same_certificates(qp, X0 * .8, frontier[6:7], _device_solve(qp, X0 * .8, frontier[6:7]), 'certify 1')

    # the search's own block: begin with a cover (two leaves per tree, the root's children, with rows), run, results, leaves
    from warm_start_hmpc_amd.batched import NodeArrays
    from warm_start_hmpc_amd.search import DeviceSearch
    from test_gpu_search import _solver
    rng = np.random.default_rng(7)
    x0s = np.array([X0, X0 * .8])
    covers = []
    for k in range(2):
        f = np.full((2, nfix), -1, np.int8)
        f[:, 0] = [0, 1]
        covers.append((f, np.zeros(2), rng.uniform(0., 1., (2, d['n_dual'])), rng.uniform(0., 1., 2)))
    ref = sr.Search(d, 2, 1024, 2048)
    ref.begin(x0s, covers)
    ds = DeviceSearch(ctrl, 2, node_cap=1024, row_cap=2048)
    ds.begin(x0s, [NodeArrays(np.ascontiguousarray(f), np.ascontiguousarray(l), dual, dobj, np.ones(len(l), bool)) for f, l, dual, dobj in covers])
    sr.compare_dicts(ref.leaves(), ds.leaves_flat(), what='cover')
    rounds, launched = ref.run(_solver(qp, ref, False), 8, 0., False)
    assert ds.run(8, 0., False) == (rounds, launched) and rounds > 1
    got = ds.results()
    sr.compare_dicts(ref.results(), got, what='results')
    assert np.array_equal(got['state'], [sr.DONE | sr.INCUMBENT] * 2) and np.isfinite(got['cost']).all()
    sr.compare_dicts(ref.leaves(), ds.leaves_flat(), what='leaves')
    for k in range(2):
        sr.compare_tree(ref.tree(k), ds.tree(k), what=('tree', k))
