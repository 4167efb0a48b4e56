"""Parent -> child hand-down of active sets (``hmpc_warm``, include/hmpc.h) -- this repository's form of the reference's
optional simplex-basis hand-down (warm_start_hmpc/controller.py:260-264, 426; subproblem_solution.py:37-43): a child node
receives its parent's record and tries the parent's active set before its first interior-point iteration.

What must hold: statuses are those of the cold solves; objectives, states and the inputs the cost sees agree (the vertex
of a verified active set does not depend on where the set came from); a child whose optimum lies on the parent's set
costs no interior-point iteration; the tree search returns the same incumbent with the same number of solves."""
import numpy as np
import pytest

from helpers import make_controller, real_tree_with_parents
from certificates import assert_certified, record_from_device

X0 = np.array([0., 0., 1., 0.])


def _handed_down(ctrl, fix, parent, cold):
    ok = (parent >= 0) & (cold['status'][np.maximum(parent, 0)] == 0) & (cold['polished'][np.maximum(parent, 0)] > 0)
    index = np.where(ok, parent, -1).astype(np.int32)
    return index, ctrl.qp.solve_batch(X0, fix, warm=(cold['primal'], cold['dual'], index))


def _check(ctrl, fix, index, cold, warm, T, min_hits):
    nx = ctrl.mld.nx
    assert np.array_equal(cold['status'], warm['status'])
    opt = cold['status'] == 0
    np.testing.assert_allclose(warm['obj'][opt], cold['obj'][opt], rtol=1e-9, atol=1e-12)
    xs = slice(0, (T + 1) * nx)
    assert np.max(np.abs(warm['primal'][opt][:, xs] - cold['primal'][opt][:, xs])) < 1e-7
    inf = cold['status'] == 1                                            # nothing is handed to a ray: bit-equal records
    assert np.array_equal(warm['dual'][inf], cold['dual'][inf]) and np.array_equal(warm['iters'][inf], cold['iters'][inf])
    handed = opt & (index >= 0)
    hits = handed & (warm['iters'] == 0)
    assert hits.sum() >= min_hits * handed.sum(), (hits.sum(), handed.sum())
    assert np.all(warm['polished'][hits] > 0)
    none = index < 0                                                     # nodes without a parent record: the cold solve
    assert np.array_equal(warm['obj'][none], cold['obj'][none]) and np.array_equal(warm['iters'][none], cold['iters'][none])
    return int(hits.sum()), int(handed.sum())


@pytest.mark.parametrize('fixture,T', [('cart_pole_with_walls', 20), ('cart_pole_with_walls', 10), ('cart_pole_one_wall', 40)])
def test_handed_down_active_sets_on_the_oracle(fixture, T):
    ctrl = make_controller(fixture, T=T, backend='oracle', threads=8)
    x0 = np.array([0., 0., .5, 0.]) if T == 10 else X0
    fix, parent = real_tree_with_parents(ctrl, x0)
    cold = ctrl.qp.solve_batch(x0, fix)
    ok = (parent >= 0) & (cold['status'][np.maximum(parent, 0)] == 0) & (cold['polished'][np.maximum(parent, 0)] > 0)
    index = np.where(ok, parent, -1).astype(np.int32)
    warm = ctrl.qp.solve_batch(x0, fix, warm=(cold['primal'], cold['dual'], index))
    hits, handed = _check(ctrl, fix, index, cold, warm, T, min_hits=0.5)
    opt = cold['status'] == 0
    assert warm['iters'][opt].mean() < 0.5 * cold['iters'][opt].mean()  # the target of the hand-down: optimal children >= 2x


def test_tree_search_with_hand_down_on_the_oracle():
    ctrl = make_controller('cart_pole_with_walls', backend='oracle', threads=1)
    a = ctrl.feedforward(X0, printing_period=None)
    b = ctrl.feedforward(X0, printing_period=None, handdown=True)
    # same incumbent; solves and leaves within 3: where the multipliers of dependent active rows are not unique (SURVEY
    # Appendix A.4) a handed-down solve may return another optimal choice than a cold one, child bounds parent + multiplier
    # then meet in another order (the reference's own published counts wobble 158..161).  Equal until the
    # round-4 changes of the oracle's arithmetic (160 / 161 since).
    assert abs(a[2] - b[2]) <= 3 and abs(len(a[1]) - len(b[1])) <= 3
    assert abs(a[0].objective - b[0].objective) <= 1e-12
    assert np.array_equal(np.concatenate(a[0].variables['ub']), np.concatenate(b[0].variables['ub']))
    assert np.max(np.abs(np.array(a[0].variables['x']) - np.array(b[0].variables['x']))) < 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize('fixture,T', [('cart_pole_with_walls', 20), ('cart_pole_with_walls', 40), ('cart_pole_one_wall', 40)])
def test_handed_down_active_sets_on_the_gpu(fixture, T):
    hip = make_controller(fixture, T=T, backend='hip')
    orc = make_controller(fixture, T=T, backend='oracle', threads=8)
    fix, parent = real_tree_with_parents(orc, X0)
    cold = hip.qp.solve_batch(X0, fix)
    ok = (parent >= 0) & (cold['status'][np.maximum(parent, 0)] == 0) & (cold['polished'][np.maximum(parent, 0)] > 0)
    index = np.where(ok, parent, -1).astype(np.int32)
    warm = hip.qp.solve_batch(X0, fix, warm=(cold['primal'], cold['dual'], index))
    hits, handed = _check(hip, fix, index, cold, warm, T, min_hits=0.5)
    assert np.array_equal(warm['handed'] > 0, (warm['iters'] == 0) & (index >= 0) & (cold['status'] == 0))
    # the same hand-down on the oracle: same nodes verify, same vertices
    oc = orc.qp.solve_batch(X0, fix)
    ow = orc.qp.solve_batch(X0, fix, warm=(oc['primal'], oc['dual'], index))
    assert np.array_equal(ow['status'], warm['status'])
    assert np.mean((ow['iters'] == 0) == (warm['iters'] == 0)) > 0.97
    opt = cold['status'] == 0
    nxs = (T + 1) * hip.mld.nx
    assert np.max(np.abs(ow['primal'][opt][:, :nxs] - warm['primal'][opt][:, :nxs])) < 1e-6
    # the handed-down records certify themselves (multipliers included: they become the next step's bounds), the oracle's
    # records of the same hand-down being the reference; and so do the cold ones
    assert_certified(hip, X0, fix, warm, ref=ow, what='handed down')
    assert_certified(hip, X0, fix, cold, ref=oc, what='cold')


@pytest.mark.gpu
def test_hand_down_in_the_device_pointer_form_and_in_the_tree_search():
    import torch
    hip = make_controller('cart_pole_with_walls', backend='hip')
    fix, parent = real_tree_with_parents(hip, X0)
    cold = hip.qp.solve_batch(X0, fix)
    ok = (parent >= 0) & (cold['status'][np.maximum(parent, 0)] == 0) & (cold['polished'][np.maximum(parent, 0)] > 0)
    index = np.where(ok, parent, -1).astype(np.int32)
    host = hip.qp.solve_batch(X0, fix, warm=(cold['primal'], cold['dual'], index))
    dev = torch.device('cuda')
    B = len(fix)
    out = dict(obj=torch.empty(B, dtype=torch.float64, device=dev), dual_obj=torch.empty(B, dtype=torch.float64, device=dev),
               status=torch.empty(B, dtype=torch.int32, device=dev), iters=torch.empty(B, dtype=torch.int32, device=dev),
               primal=torch.empty(B, hip.qp.n_primal, dtype=torch.float64, device=dev),
               dual=torch.empty(B, hip.qp.n_dual, dtype=torch.float64, device=dev))
    wp, wd, wi = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (cold['primal'], cold['dual'], index))
    hip.qp.solve_batch_device(torch.from_numpy(X0).to(dev), torch.from_numpy(fix).to(dev), out, warm=(wp, wd, wi))
    torch.cuda.synchronize()
    assert np.array_equal(out['status'].cpu().numpy(), host['status'])
    assert np.array_equal(out['iters'].cpu().numpy() & 0xFFFF, host['iters'])
    for k in ('obj', 'dual_obj', 'primal', 'dual'):                          # same records through both entry points, to the bit
        a, b = np.ascontiguousarray(out[k].cpu().numpy()), np.ascontiguousarray(host[k])
        rows = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).reshape(B, -1).any(axis=1))
        assert rows.size == 0, (k, 'rows', rows.tolist(), 'handed', index[rows].tolist())
    orc = make_controller('cart_pole_with_walls', backend='oracle', threads=8)
    oc = orc.qp.solve_batch(X0, fix)
    ow = orc.qp.solve_batch(X0, fix, warm=(oc['primal'], oc['dual'], index))     # (the oracle's records of the same hand-down)
    assert_certified(hip, X0, fix, host, ref=ow, what='handed down, host entry')
    assert_certified(hip, X0, fix, record_from_device(*(out[k].cpu().numpy() for k in ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual'))),
                     ref=ow, what='handed down, device entry')
    # the tree search with the hand-down: same incumbent; the number of solves may move by a node or two (multipliers
    # of dependent active rows are not unique, a handed-down solve may return another optimal choice: child bounds
    # parent bound + multiplier then differ in the order equal bounds are met -- as between any two solvers)
    a = hip.feedforward(X0, printing_period=None)
    b = hip.feedforward(X0, printing_period=None, handdown=True)
    assert abs(a[2] - b[2]) <= 3 and abs(a[0].objective - b[0].objective) <= 1e-10
    assert np.array_equal(np.concatenate(a[0].variables['ub']), np.concatenate(b[0].variables['ub']))


@pytest.mark.gpu
def test_hand_down_on_the_streaming_kernel():
    # BASELINE configs[4] (random MLD nx=20, nu=6+8, N=30; the streaming form of the generic kernel, its instantiation with
    # the hand-down): the tree a dive leaves behind -- prefix chain of the first 64 binaries + one-flip siblings --, every node
    # handed its parent's record; kernel and oracle verify the same handed-down sets and return the same records
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    from bench import dive_tree
    from helpers import random_mld, _NoBackend
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    from oracle.oracle_qp import OracleBatchedQP
    mld, objective, x0 = random_mld()
    T, nub, nx = 30, 8, 20
    ctrl = HybridModelPredictiveController(mld, T, objective, None, backend=_NoBackend())
    hip, orc = HipBatchedQP(ctrl.problem_data()), OracleBatchedQP(ctrl.problem_data(), threads=8)
    Cj = np.array([mld.F[52 + 4 * j] for j in range(nub)])
    leaf = np.full((1, T * nub), -1, np.int8)
    for t in range(8):
        r = orc.solve_batch(x0, leaf)
        assert r['status'][0] == 0
        leaf[0, t * nub:(t + 1) * nub] = (r['primal'][0][:(T + 1) * nx].reshape(T + 1, nx)[t] @ Cj.T >= 0)
    short, parent = dive_tree(leaf[0, :64])
    f = np.full((len(short), T * nub), -1, np.int8)
    f[:, :64] = short
    cold_k, cold_o = hip.solve_batch(x0, f), orc.solve_batch(x0, f)
    assert np.array_equal(cold_k['status'], cold_o['status'])
    good = (parent >= 0) & (cold_o['status'][np.maximum(parent, 0)] == 0) & (cold_o['polished'][np.maximum(parent, 0)] > 0) \
        & (cold_k['polished'][np.maximum(parent, 0)] > 0)
    idx = np.where(good, parent, -1).astype(np.int32)
    a = hip.solve_batch(x0, f, warm=(cold_k['primal'], cold_k['dual'], idx))
    b = orc.solve_batch(x0, f, warm=(cold_o['primal'], cold_o['dual'], idx))
    assert np.array_equal(a['status'], b['status']) and np.array_equal(a['status'], cold_k['status'])
    assert a['handed'].sum() >= 10
    assert np.array_equal(a['handed'] > 0, b['polished'] == 64)        # (the oracle flags a verified hand-down as attempt 64)
    opt = a['status'] == 0
    np.testing.assert_allclose(a['obj'][opt], b['obj'][opt], rtol=2e-6, atol=1e-9)
    both = opt & (a['polished'] > 0) & (b['polished'] > 0)
    xs = (T + 1) * nx
    assert np.abs(a['primal'][both][:, :xs] - b['primal'][both][:, :xs]).max() < 1e-7
    assert_certified(ctrl, x0, f, a, ref=b, what='handed down, streaming kernel')
    assert a['iters'].mean() < cold_k['iters'].mean()
