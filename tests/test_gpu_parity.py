"""Parity of the HIP path (through the C ABI) with the CPU oracle and the golden vectors.

Bar (BASELINE.json north_star): statuses and binary assignments bit-exact, continuous
trajectories within 1e-5 relative -- one tolerance for every node of every configuration.
Since round 2 an optimal node returns the vertex solution of its active set (the polish of
hmpc_kernel.hip / oracle/hsde_qp.c), so the determined part of a trajectory -- states, inputs the
cost sees, every input once all binaries are fixed -- is accurate to ~1e-8; the golden vectors
come from the oracle run tighter than the product and were accepted against an independent
dense active-set solve (tests/golden/make_golden_qp.py)."""
import os

import numpy as np
import pytest

from helpers import make_controller, load_fixture, random_prefix_frontier, random_mld, dive_leaf, dive_and_prefix_frontier, _NoBackend, exercise_bounded_qp
from dense_qp import determined_inputs
from kkt_checks import check_solution, is_disjoint_cover
from certificates import assert_certified, record_from_device, new_margins, margins_line, EXTRA_LINES
from warm_start_hmpc_amd.subproblem_solution import SubproblemSolution

pytestmark = pytest.mark.gpu

X0 = np.array([0., 0., 1., 0.])
RTOL = 1e-5   # north_star: continuous trajectories within 1e-5 relative -- ONE tolerance, every node, every config


ETOL, EFLOOR = 1e-5, 1e-6   # element-wise: every component within 1e-5 of its own size (components below 1e-6: of 1e-6)
# Records WITHOUT the polished flag (HMPC_ITERS_POLISHED clear: the active-set polish did not verify, the record is an
# interior-point iterate -- a documented, distinct outcome, include/hmpc.h) are held to the SAME tolerance since round 4.
# Until round 3 such a record was the iterate at gap 1e-8 .. 1e-6 (2 - 7 % of the optimal nodes of BASELINE configs[4]),
# reproducible to ~sqrt(gap) = 1e-4 only, and this file carried an ITERATE_RTOL = 1e-3 for them.  Now a solve whose last
# polish attempt fails tightens its stopping tolerance (1e-10, then 1e-12) and tries again from the tighter iterate
# (tolerance escalation, hmpc_kernel.hip ipm_solve / oracle/hsde_qp.c solve_one): every optimal node of the configs[4]
# frontiers polishes, and the rare record that still does not is an iterate at gap 1e-12 -- compared norm-wise at RTOL
# (element-wise comparison is for vertex records: a component of 1e-6 in an iterate is not accurate to 1e-11).
WORST = {'norm': 0.0, 'element': 0.0, 'dense': 0.0, 'iterate': 0.0}   # largest deviations seen in this session (printed at the end)


def _rel(a, b, elementwise=True, efloor=None):
    """Largest deviation of a from b per row, relative to the row's largest entry of b (floor 1e-2) -- and, beside
    that norm-wise measure, the element-wise one: every component relative to its OWN size (floor EFLOOR), so that a
    small component (a pole angle of 1e-3 next to a velocity of 1) is held to the same relative accuracy."""
    if a.shape[1] == 0 or a.shape[0] == 0:
        return np.zeros(a.shape[0])
    scale = np.maximum(1e-2, np.max(np.abs(b), axis=1, keepdims=True))
    norm = np.max(np.abs(a - b) / scale, axis=1)
    if not elementwise:
        WORST['iterate'] = max(WORST['iterate'], norm.max())   # (records without the polished flag)
        return norm
    WORST['norm'] = max(WORST['norm'], norm.max())
    elem = np.max(np.abs(a - b) / np.maximum(np.abs(b), EFLOOR if efloor is None else efloor), axis=1)
    WORST['element'] = max(WORST['element'], elem.max())
    return np.maximum(norm, elem * (RTOL / ETOL))


_DENSE = {}
MARGINS = new_margins()   # certificate residuals of the kernels' records beside the oracle's, over every _compare of this session


@pytest.fixture(scope='module', autouse=True)
def _report_worst_deviations():
    yield
    line = ('parity margins of this run: kernel vs oracle norm-wise %.2e, element-wise (floor %.0e) %.2e; kernel vs dense '
            'active-set solve %.2e; unpolished records (interior-point iterates) norm-wise %.2e'
            % (WORST['norm'], EFLOOR, WORST['element'], WORST['dense'], WORST['iterate']))
    line += '; ' + margins_line(MARGINS)
    line = '\n'.join([line] + EXTRA_LINES)                  # (what modules that ran before this one left: tests/test_gpu_enumerated_miqp.py)
    print('\n' + line)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
    if os.path.isdir(out):
        with open(os.path.join(out, 'parity_margins.txt'), 'a') as f:
            f.write(line + '\n')


def _dense_check(ctrl, T, x0, fix, rec, sample=64, seed=0):
    """The kernel's optimal records against the dense active-set solve (tests/dense_qp.py: numpy SVD on the dense
    statement of the node QP, no code shared with oracle or kernel) -- a seeded sample per call, states to 1e-7."""
    from dense_qp import dense_qp, active_set_primal
    key = id(ctrl)
    if getattr(ctrl, '_dense_qp_of_the_parity_tests', None) is None:   # (kept on the controller: id() of a collected one is reused)
        ctrl._dense_qp_of_the_parity_tests = dense_qp(ctrl)
    _DENSE[key] = ctrl._dense_qp_of_the_parity_tests
    opt = np.flatnonzero((rec['status'] == 0) & (rec['polished'] > 0))
    if opt.size > sample:
        opt = np.random.RandomState(seed).choice(opt, sample, replace=False)
    nxs = (T + 1) * ctrl.mld.nx
    x0 = np.asarray(x0)
    for i in opt:
        w, resid = active_set_primal(ctrl, _DENSE[key], x0 if x0.ndim == 1 else x0[i], np.asarray(fix)[i], rec['dual'][i])
        assert resid < 1e-9, resid
        dev = np.max(np.abs(w[:nxs] - rec['primal'][i][:nxs])) / max(1e-2, np.max(np.abs(w[:nxs])))
        WORST['dense'] = max(WORST['dense'], dev)
        assert dev < 1e-7, ('dense active-set solve', int(i), dev)
    return opt.size


def _trajectories_close(ctrl, T, fix, pa, pb, what='', elementwise=True, efloor=None):
    """States, the inputs the cost is strictly convex in (unique at every node), and -- where every binary is
    fixed, the nodes an incumbent comes from -- ALL inputs, at RTOL.  Inputs no cost term sees are not unique in
    a relaxation: a vertex solution and Gurobi's would differ there as well."""
    nx, nu = ctrl.mld.nx, ctrl.mld.nu
    xa, xb = pa[:, :(T + 1) * nx], pb[:, :(T + 1) * nx]
    ua, ub = pa[:, (T + 1) * nx:].reshape(-1, T, nu), pb[:, (T + 1) * nx:].reshape(-1, T, nu)
    # (element-wise -- every component to 1e-5 of its own size -- where both sides return the vertex of an active set;
    # an interior-point iterate that meets the stopping test is compared norm-wise only)
    assert _rel(xa, xb, elementwise, efloor).max(initial=0) < RTOL, (what, 'x', _rel(xa, xb, elementwise, efloor).max())
    for j in determined_inputs(ctrl):
        assert _rel(ua[:, :, j], ub[:, :, j], elementwise, efloor).max(initial=0) < RTOL, (what, 'u', j, _rel(ua[:, :, j], ub[:, :, j], elementwise, efloor).max())
    if fix is not None:
        full = (np.asarray(fix) >= 0).all(axis=1)
        if full.any():
            assert _rel(ua[full].reshape(full.sum(), -1), ub[full].reshape(full.sum(), -1), elementwise, efloor).max() < RTOL, (what, 'u of fully fixed nodes')


def _compare(ctrl, a, b, T, fix=None, min_polished=1.0, x0=None, efloor=None):
    """a: records of the HIP path, b: of the oracle.  With x0 (and fix) the polished records of the HIP path are also
    checked against the dense active-set solve, which shares no code with either, and EVERY record of the HIP path is held to
    its own certificate (tests/certificates.py: KKT point or Farkas ray, from the rows as written out), the oracle's records of
    the same workload being the reference."""
    assert np.array_equal(a['status'], b['status']), np.flatnonzero(a['status'] != b['status'])
    if x0 is not None and fix is not None:
        _dense_check(ctrl, T, x0, fix, a)
        assert_certified(ctrl, x0, fix, a, ref=b, margins=MARGINS)
    assert np.all(a['status'] <= 1)
    fin = a['status'] == 0
    # polished on both sides (every optimal node of the cart-pole systems): vertex solutions, objectives to 1e-8;
    # where the polish did not verify (hard relaxations of the random MLD) both sides return the interior-point
    # iterate: objectives to the solver's tolerance (1e-8 gap, 1e-6 through the exhausted-barrier exit)
    pol = fin & (a['polished'] > 0) & (b['polished'] > 0)
    raw = fin & ~pol
    np.testing.assert_allclose(a['obj'][pol], b['obj'][pol], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(a['dual_obj'][pol], b['dual_obj'][pol], rtol=1e-6, atol=1e-9)   # (evaluated from multipliers of order 1e2)
    np.testing.assert_allclose(a['obj'][raw], b['obj'][raw], rtol=1e-8, atol=1e-11)      # (iterates at gap <= 1e-10 since round 4)
    np.testing.assert_allclose(a['dual_obj'][raw], b['dual_obj'][raw], rtol=1e-6, atol=1e-9)
    if min_polished is not None:   # (one record is always allowed for: 48-node frontiers have ~40 optimal nodes)
        assert pol.sum() >= min(min_polished * fin.sum(), fin.sum() - 1), (pol.sum(), fin.sum())
    _trajectories_close(ctrl, T, None if fix is None else np.asarray(fix)[pol], a['primal'][pol], b['primal'][pol], 'polished', efloor=efloor)
    _trajectories_close(ctrl, T, None if fix is None else np.asarray(fix)[raw], a['primal'][raw], b['primal'][raw], 'iterate', elementwise=False)
    inf = a['status'] == 1
    assert np.all(np.isinf(a['obj'][inf])) and np.all(np.isnan(a['primal'][inf]))
    # Farkas rays are normalised to a unit largest multiplier on both sides
    np.testing.assert_allclose(a['dual'][inf], b['dual'][inf], rtol=0, atol=1e-6)
    np.testing.assert_allclose(a['dual_obj'][inf], b['dual_obj'][inf], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize('fixture,T,terminal,count,p_one', [
    ('cart_pole_with_walls', 20, True, 256, 0.1),
    ('cart_pole_with_walls', 20, True, 256, 0.5),
    ('cart_pole_with_walls', 10, True, 128, 0.1),
    ('cart_pole_with_walls', 10, False, 64, 0.1),
    ('cart_pole_with_walls', 40, True, 48, 0.05),
    ('cart_pole_one_wall', 40, True, 96, 0.1),
])
def test_frontier_parity_with_oracle(fixture, T, terminal, count, p_one):
    hip = make_controller(fixture, T=T, terminal=terminal, backend='hip')
    orc = make_controller(fixture, T=T, terminal=terminal, backend='oracle', threads=8)
    fix = random_prefix_frontier(T, hip.mld.nub, count, p_one=p_one)
    fix[0, :] = -1
    x0 = np.array([0., 0., .5, 0.]) if T == 10 and terminal else X0
    _compare(hip, hip.qp.solve_batch(x0, fix), orc.qp.solve_batch(x0, fix), T, fix, x0=x0)


@pytest.mark.parametrize('waves', ['1', '2', '4'])
@pytest.mark.parametrize('fixture,T', [('cart_pole_with_walls', 20), ('cart_pole_with_walls', 40), ('cart_pole_one_wall', 40)])
def test_every_kernel_instantiation(monkeypatch, fixture, T, waves):
    # 1 / 2 / 4 waves per node select different compile-time kernels (row-slot layouts differ with the
    # number of lanes); the batch-size rule would only ever pick one of them for a test-sized frontier
    hip = make_controller(fixture, T=T, backend='hip')
    orc = make_controller(fixture, T=T, backend='oracle', threads=8)
    fix = random_prefix_frontier(T, hip.mld.nub, 40, p_one=0.1, seed0=9000)
    fix[0, :] = -1
    monkeypatch.setenv('HMPC_WAVES', waves)
    res = hip.qp.solve_batch(X0, fix)
    monkeypatch.delenv('HMPC_WAVES')
    _compare(hip, res, orc.qp.solve_batch(X0, fix), T, fix, x0=X0)


def test_shallow_wide_family_polishes_everywhere():
    # the nodes whose active sets need the second penalty level of the polish (see the CPU test of the same family):
    # kernel == oracle at RTOL, every optimal node polished on both sides, and the kernel's records against the dense
    # active-set solve, which shares no code with either
    from helpers import shallow_wide_family
    from dense_qp import dense_qp, active_set_primal
    x0, fix = shallow_wide_family('cart_pole_one_wall', 40, 4000, .6)
    hip = make_controller('cart_pole_one_wall', T=40, backend='hip')
    orc = make_controller('cart_pole_one_wall', T=40, backend='oracle', threads=8)
    a, b = hip.qp.solve_batch(x0, fix), orc.qp.solve_batch(x0, fix)
    _compare(hip, a, b, 40, fix, x0=x0)
    opt = np.flatnonzero(a['status'] == 0)
    assert opt.size > 300 and np.all(a['polished'][opt] > 0)
    dq = dense_qp(hip)
    late = opt[np.argsort(-(a['iters'][opt] & 0xFFFF))][:40]
    for i in np.concatenate((late, opt[:40])):
        w, resid = active_set_primal(hip, dq, x0[i], fix[i], a['dual'][i])
        n = 41 * 4
        assert resid < 1e-10
        assert np.max(np.abs(w[:n] - a['primal'][i][:n])) / max(1e-2, np.max(np.abs(w[:n]))) < 1e-7


def test_generic_kernel_forced_on_cart_pole(monkeypatch):
    # the run-time-sized kernel (list row map, LDS factor) on the reference's system
    monkeypatch.setenv('HMPC_FORCE_GENERIC', '1')
    hip = make_controller('cart_pole_with_walls', backend='hip')
    monkeypatch.delenv('HMPC_FORCE_GENERIC')
    orc = make_controller('cart_pole_with_walls', backend='oracle', threads=8)
    for count in (32, 600):                                  # 4 waves and 1 wave per node
        fix = random_prefix_frontier(20, 4, count, p_one=0.2, seed0=11000)
        fix[0, :] = -1
        _compare(hip, hip.qp.solve_batch(X0, fix), orc.qp.solve_batch(X0, fix), 20, fix, x0=X0)


def test_per_node_initial_states():
    hip = make_controller('cart_pole_with_walls', T=10, backend='hip')
    orc = make_controller('cart_pole_with_walls', T=10, backend='oracle', threads=8)
    rng = np.random.default_rng(5)
    fix = random_prefix_frontier(10, 4, 96, p_one=0.05)
    x0 = rng.uniform(-1, 1, (96, 4)) * np.array([.3, .1, .6, .4])
    _compare(hip, hip.qp.solve_batch(x0, fix), orc.qp.solve_batch(x0, fix), 10, fix, x0=x0)


def test_golden_vectors():
    g = load_fixture('qp_golden')
    for name, fixture in [('n20', 'cart_pole_with_walls'), ('n20dive', 'cart_pole_with_walls'),
                          ('n20tree', 'cart_pole_with_walls'), ('n20x0', 'cart_pole_with_walls'),
                          ('n10', 'cart_pole_with_walls'), ('n10free', 'cart_pole_with_walls'),
                          ('n40', 'cart_pole_with_walls'), ('onewall', 'cart_pole_one_wall')]:
        T = int(g[name + '_T'])
        ctrl = make_controller(fixture, T=T, terminal=bool(g[name + '_terminal']), backend='hip')
        res = ctrl.qp.solve_batch(g[name + '_x0'], g[name + '_fix'])
        assert np.array_equal(res['status'], g[name + '_status']), name
        fin = res['status'] == 0
        np.testing.assert_allclose(res['obj'][fin], g[name + '_obj'][fin], rtol=1e-8, atol=1e-11)
        ref = np.hstack((g[name + '_x'], g[name + '_u']))
        _trajectories_close(ctrl, T, g[name + '_fix'][fin], res['primal'][fin], ref[fin], name)
        assert_certified(ctrl, g[name + '_x0'], g[name + '_fix'], res, what=name)   # (no oracle record in the file: base tolerances)
        if name + '_bb_ub' not in g:
            continue
        # the whole branch and bound through the GPU path: binary assignment bit-exact, the incumbent's
        # trajectory (states and continuous inputs) at RTOL
        sol, leaves, solves, _ = ctrl.feedforward(g[name + '_x0'], printing_period=None)
        assert abs(len(leaves) - int(g[name + '_bb_leaves'])) <= 2 and abs(solves - int(g[name + '_bb_solves'])) <= 4
        assert abs(sol.objective - float(g[name + '_bb_cost'])) <= 1e-8 * (1 + abs(sol.objective))
        if not np.array_equal(np.array(sol.variables['ub']), g[name + '_bb_ub']):
            # only legitimate for a TIE of the MIQP (n10free has one: without a terminal set the damper binary of the
            # last stages is free of charge): the golden assignment must then be exactly as good on this path
            tie = ctrl.qp.solve_batch(g[name + '_x0'], g[name + '_bb_ub'].astype(np.int8).reshape(1, -1))
            assert name == 'n10free' and tie['status'][0] == 0 and abs(tie['obj'][0] - sol.objective) <= 1e-12 * (1 + sol.objective), name
        for key in ('x', 'uc'):
            got, want = np.array(sol.variables[key]).reshape(1, -1), g[name + '_bb_' + key].reshape(1, -1)
            # (element-wise floor 1e-5 on the one-wall system: its cost has a curvature of order one, the polish runs at its second
            # penalty level throughout (DevProb::polish_l1, round 4) and a vertex is good to ~1e-10 absolute instead of 1e-12:
            # measured 1.0e-11 on a component of 1e-7; norm-wise the same 1e-9)
            fl = 1e-5 if name == 'onewall' else None
            assert _rel(got, want, True, fl).max() < RTOL, (name, 'incumbent', key, _rel(got, want, True, fl).max())


def test_full_size_frontier_certifies_itself():
    # BASELINE.json configs[2] size: 1024 nodes; size-independent property = every record is a
    # KKT point or a Farkas proof by the reference's own checkers
    ctrl = make_controller('cart_pole_with_walls', backend='hip')
    fix = random_prefix_frontier(20, 4, 1024, p_one=0.1)
    res = ctrl.qp.solve_batch(X0, fix)
    assert np.all(res['status'] <= 1)
    kinds = {'optimal': 0, 'infeasible': 0}
    for b in range(0, 1024):
        sol = SubproblemSolution.from_rows(ctrl.layout, fix[b], res['obj'][b], res['dual_obj'][b], res['status'][b],
                                           res['primal'][b], res['dual'][b])
        ident = {(k // 4, k % 4): float(v) for k, v in enumerate(fix[b]) if v >= 0}
        kinds[check_solution(ctrl, sol, ident, X0, tol=1e-8 if res['status'][b] == 0 else 1e-6)] += 1
    assert kinds['optimal'] > 50 and kinds['infeasible'] > 500
    # monotonicity along a chain: fixing more binaries never lowers the optimum
    chain = np.full((21, 80), -1, dtype=np.int8)
    for k in range(1, 21):
        chain[k, :4 * k] = 0
    obj = ctrl.qp.solve_batch(np.array([0., 0., .2, 0.]), chain)['obj']
    assert np.all(np.diff(obj) >= -1e-8)


def test_result_is_independent_of_batch_position_and_size():
    ctrl = make_controller('cart_pole_with_walls', backend='hip')
    fix = random_prefix_frontier(20, 4, 700, p_one=0.1)    # more nodes than resident workgroups
    a = ctrl.qp.solve_batch(X0, fix)
    perm = np.random.default_rng(0).permutation(700)
    b = ctrl.qp.solve_batch(X0, fix[perm])
    for k in ('obj', 'dual_obj', 'status', 'iters', 'dual'):
        assert np.array_equal(a[k][perm], b[k], equal_nan=True), k         # bitwise: position in the batch
    # bitwise also across batch sizes that use the same launch configuration (all branch-and-bound
    # rounds are in this class: the exact warm == cold objective of test_controller.py:165-170 relies on it)
    c, d = ctrl.qp.solve_batch(X0, fix[:1]), ctrl.qp.solve_batch(X0, fix[:40])
    assert c['obj'][0] == d['obj'][0] and np.array_equal(c['dual'][0], d['dual'][0], equal_nan=True)
    assert np.array_equal(d['primal'][:40], ctrl.qp.solve_batch(X0, fix[:200])['primal'][:40], equal_nan=True)
    # across launch configurations (waves per node follow the batch size) the reduction trees differ:
    # same statuses, values equal to solver accuracy
    assert np.array_equal(a['status'][:40], d['status'])
    fin = d['status'] == 0
    np.testing.assert_allclose(a['obj'][:40][fin], d['obj'][fin], rtol=2e-6, atol=1e-9)


def test_edge_cases():
    ctrl = make_controller('cart_pole_with_walls', T=10, backend='hip')
    x0 = np.array([0., 0., .5, 0.])
    empty = ctrl.qp.solve_batch(x0, np.zeros((0, 40), dtype=np.int8))
    assert empty['obj'].shape == (0,)
    full = np.zeros((3, 40), dtype=np.int8)                 # every binary fixed (binary feasible nodes)
    full[1, 3] = 1
    full[2, :] = 1
    res = ctrl.qp.solve_batch(x0, full)
    assert res['status'][0] == 0 and abs(res['obj'][0] - 0.0995300) < 1e-6
    assert res['status'][2] == 1
    far = ctrl.qp.solve_batch(np.array([0., 0., 5., 0.]), np.full((2, 40), -1, dtype=np.int8))   # state outside the box
    assert np.all(far['status'] == 1)
    with pytest.raises(ValueError):
        ctrl.qp.solve_batch(x0, np.zeros((2, 39), dtype=np.int8))
    with pytest.raises(ValueError):
        ctrl.qp.solve_batch(np.zeros(3), np.zeros((2, 40), dtype=np.int8))
    only_obj = ctrl.qp.solve_batch(x0, full, want_primal=False, want_dual=False)
    assert only_obj['primal'] is None and np.array_equal(only_obj['obj'], res['obj'])


def test_device_pointer_entry_point_matches_host_one():
    import torch
    ctrl = make_controller('cart_pole_with_walls', backend='hip')
    fix = random_prefix_frontier(20, 4, 300, p_one=0.1)
    ref = ctrl.qp.solve_batch(X0, fix)
    dev = torch.device('cuda', 0)
    out = dict(obj=torch.empty(300, dtype=torch.float64, device=dev), dual_obj=torch.empty(300, dtype=torch.float64, device=dev),
               status=torch.empty(300, dtype=torch.int32, device=dev), iters=torch.empty(300, dtype=torch.int32, device=dev),
               primal=torch.empty(300, ctrl.qp.n_primal, dtype=torch.float64, device=dev),
               dual=torch.empty(300, ctrl.qp.n_dual, dtype=torch.float64, device=dev))
    ctrl.qp.solve_batch_device(torch.from_numpy(X0).to(dev), torch.from_numpy(fix).to(dev), out)
    torch.cuda.synchronize()
    for k in ('obj', 'dual_obj', 'status', 'primal', 'dual'):
        assert np.array_equal(out[k].cpu().numpy(), ref[k], equal_nan=True), k
    assert np.array_equal(out['iters'].cpu().numpy() & 0xFFFF, ref['iters'])        # bit 16: HMPC_ITERS_POLISHED
    assert np.array_equal((out['iters'].cpu().numpy() >> 16) & 1, ref['polished'])


def test_branch_and_bound_and_warm_start_on_gpu():
    hip = make_controller('cart_pole_with_walls', backend='hip')
    orc = make_controller('cart_pole_with_walls', backend='oracle')
    sol, leaves, solves, _ = hip.feedforward(X0, printing_period=None)
    ref = orc.feedforward(X0, printing_period=None)
    assert np.array_equal(np.array(sol.variables['ub']), np.array(ref[0].variables['ub']))     # bit-exact binaries
    assert abs(sol.objective - ref[0].objective) < 1e-8 * (1 + abs(ref[0].objective))
    for key in ('x', 'uc'):                                                                      # the incumbent's trajectory
        got, want = np.array(sol.variables[key]).reshape(1, -1), np.array(ref[0].variables[key]).reshape(1, -1)
        assert _rel(got, want).max() < RTOL, (key, _rel(got, want).max())
    assert 157 <= solves <= 162 and len(leaves) == 81 and is_disjoint_cover(hip, leaves)      # published 158-161
    x, ws = X0, None
    for step in range(4):
        cold = hip.feedforward(x, printing_period=None)
        warm = hip.feedforward(x, printing_period=None, warm_start=ws)
        wide = hip.feedforward(x, printing_period=None, warm_start=None, frontier_width=16)
        assert warm[0].objective == cold[0].objective == wide[0].objective                     # test_controller.py:165-170
        if step:
            assert warm[2] <= 25
        ws = hip.construct_warm_start(warm[1], x, warm[0].variables['uc'][0], warm[0].variables['ub'][0], np.zeros(4))[0]
        assert len(ws) == 77
        x = warm[0].variables['x'][1]


def test_other_problem_shapes_and_size_limit():
    # a small random MLD exercises nx, nu, nub, row counts unlike the cart-pole's
    mld, objective, x0 = random_mld(nx=6, nuc=2, nub=3, seed=3)
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    from oracle.oracle_qp import OracleBatchedQP
    ctrl = HybridModelPredictiveController(mld, 8, objective, None, backend=_NoBackend())
    hip, orc = HipBatchedQP(ctrl.problem_data()), OracleBatchedQP(ctrl.problem_data(), threads=8)
    fix = random_prefix_frontier(8, 3, 128, p_one=0.3)
    fix[0, :] = -1
    _compare(ctrl, hip.solve_batch(x0, fix), orc.solve_batch(x0, fix), 8, fix, min_polished=0.99, x0=x0)


def test_register_kernel_compiled_for_an_arbitrary_shape():
    # a shape without a built-in instantiation gets the register kernel, compiled at hmpc_create (csrc/hmpc_jit.h): same
    # results as the oracle at the one tolerance (and as the run-time-sized kernel, which served such shapes until round 4)
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    from oracle.oracle_qp import OracleBatchedQP
    # (the last three: nx + nu = 16 -- the full row of 16 lanes; until round 5 every node of such a problem ended NUMERICAL,
    # the LDS carve of the register kernels at nz >= 16 -- and a problem whose one-wave binary round 4 saw come out wrong)
    for (nx, nuc, nub, T, seed) in ((6, 2, 3, 8, 3), (8, 3, 4, 10, 2), (9, 3, 4, 6, 23), (8, 4, 4, 6, 23), (3, 3, 6, 12, 38)):
        mld, objective, x0 = random_mld(nx=nx, nuc=nuc, nub=nub, seed=seed)
        ctrl = HybridModelPredictiveController(mld, T, objective, None, backend=_NoBackend())
        hip, orc = HipBatchedQP(ctrl.problem_data()), OracleBatchedQP(ctrl.problem_data(), threads=8)
        assert hip.kernel_info() == (6, 6, 6), hip.kernel_info()   # (compiled with the problem's sizes; 3: per shape, HMPC_JIT_SIZED=0)
        fix = dive_and_prefix_frontier(orc, mld, x0, T, seed)
        for waves in ('1', '2', '4'):
            os.environ['HMPC_WAVES'] = waves
            try:
                a = hip.solve_batch(x0, fix)
            finally:
                del os.environ['HMPC_WAVES']
            b = orc.solve_batch(x0, fix)
            assert (a['status'] == 0).sum() >= 20 and (a['status'] == 1).sum() >= 20
            _compare(ctrl, a, b, T, fix, min_polished=0.99, x0=x0, efloor=1e-5)
        os.environ['HMPC_JIT'] = '0'
        try:
            gen = HipBatchedQP(ctrl.problem_data())
        finally:
            del os.environ['HMPC_JIT']
        assert gen.kernel_info() == (0, 0, 0)
        g = gen.solve_batch(x0, fix)
        assert np.array_equal(g['status'], a['status'])
        fin = a['status'] == 0
        np.testing.assert_allclose(g['obj'][fin], a['obj'][fin], rtol=1e-8, atol=1e-11)


@pytest.mark.parametrize('which', [1, 2])
def test_sized_kernels_of_a_problem_beyond_the_static_row_map(which):
    # nx + nu = 18 / 19: no register kernel (the static row map ends at 16), the problem fits one CU's LDS -- the run-time-sized
    # kernel compiled with the problem's sizes serves 1 / 2 / 4 waves per node (csrc/hmpc_jit.h, round 4).  Same records as
    # the oracle at the one tolerance, and as the shipped run-time-sized kernel (HMPC_JIT_SIZED=0).
    from jit_problems import problem, SIZED
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    from oracle.oracle_qp import OracleBatchedQP
    nx, nuc, nub, seed, T = SIZED[which]
    data, mld, objective, x0 = problem(*SIZED[which])
    ctrl = HybridModelPredictiveController(mld, T, objective, None, backend=_NoBackend())
    hip, orc = HipBatchedQP(data), OracleBatchedQP(data, threads=8)
    assert hip.kernel_info() == (4, 4, 4), hip.kernel_info()
    os.environ['HMPC_JIT_SIZED'] = '0'
    try:
        plain = HipBatchedQP(data)
    finally:
        del os.environ['HMPC_JIT_SIZED']
    assert plain.kernel_info() == (0, 0, 0)
    fix = dive_and_prefix_frontier(orc, mld, x0, T, seed)
    b = orc.solve_batch(x0, fix)
    assert (b['status'] == 0).sum() >= 20 and (b['status'] == 1).sum() >= 20
    for waves in ('1', '2', '4'):
        os.environ['HMPC_WAVES'] = waves
        try:
            a, c = hip.solve_batch(x0, fix), plain.solve_batch(x0, fix)
        finally:
            del os.environ['HMPC_WAVES']
        _compare(ctrl, a, b, T, fix, min_polished=0.99, x0=x0, efloor=1e-5)
        assert np.array_equal(c['status'], a['status'])
        fin = a['status'] == 0
        np.testing.assert_allclose(c['obj'][fin], a['obj'][fin], rtol=1e-9, atol=1e-12)


def test_compiled_kernels_are_checked_at_their_first_launch(monkeypatch, capfd):
    # A kernel compiled at hmpc_create is code nobody has run before: the first launch through it solves the first nodes of its
    # batch with the shipped kernel of the same wave count as well and compares (hmpc_capi.hip: hmpc_check_compiled).  Agreement
    # keeps it; a disagreement (forced here by the test hook) drops it for the handle, loudly, and the shipped kernel serves --
    # same records either way.
    x0 = np.array([0., 0., .5, 0.])
    fix = random_prefix_frontier(10, 4, 24, p_one=0.1)
    fix[0, :] = -1
    good = make_controller('cart_pole_with_walls', T=10, backend='hip')
    a = good.qp.solve_batch(x0, fix)
    assert good.qp.kernel_info() == (6, 6, 6)
    assert 'disagrees' not in capfd.readouterr().err
    monkeypatch.setenv('HMPC_JIT_SELFCHECK_FAIL', '1')
    bad = make_controller('cart_pole_with_walls', T=10, backend='hip')
    assert bad.qp.kernel_info() == (6, 6, 6)
    b = bad.qp.solve_batch(x0, fix)                                        # (24 nodes: four waves per node)
    monkeypatch.delenv('HMPC_JIT_SELFCHECK_FAIL')
    assert bad.qp.kernel_info() == (6, 6, 2), bad.qp.kernel_info()         # dropped where it was launched, and only there
    assert 'disagrees with the shipped kernel' in capfd.readouterr().err
    assert np.array_equal(a['status'], b['status'])
    fin = a['status'] == 0
    np.testing.assert_allclose(a['obj'][fin], b['obj'][fin], rtol=1e-9, atol=1e-12)
    c = bad.qp.solve_batch(x0, fix)                                        # the shipped kernel from then on: bit-equal to itself
    assert np.array_equal(b['obj'], c['obj'])


def test_register_kernel_on_the_bench_workload_of_generic_vs_specialised():
    # bench.py's `generic_vs_specialised` workload -- random MLD nx = 6, nu = 2 + 3, N = 12, 2048 random
    # prefixes (p_one 0.3), node 0 the root -- showed the register kernel compiled for the problem leaving 1 node undecided and 3
    # optimal nodes unpolished where the run-time-sized kernel and the oracle decide and polish all 178: the multipliers a
    # stationarity row of the step defines were taken from the accumulated solves in the register kernels (hmpc_kernel.hip, top:
    # one feature set for every kernel).  EXACTLY that workload, without the nets: register kernel == oracle == run-time-sized
    # kernel at the one tolerance, no node undecided, every optimal node polished on all three, at 1 / 2 / 4 waves per node.
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    from oracle.oracle_qp import OracleBatchedQP
    mld, objective, x0 = random_mld(nx=6, nuc=2, nub=3, seed=3)
    T = 12
    ctrl = HybridModelPredictiveController(mld, T, objective, None, backend=_NoBackend())
    fix = random_prefix_frontier(T, 3, 2048, p_one=0.3)
    fix[0, :] = -1
    data = ctrl.problem_data()
    b = OracleBatchedQP(data, threads=16).solve_batch(x0, fix)
    assert np.all(b['status'] <= 1) and (b['status'] == 0).sum() == 178 and np.all(b['polished'][b['status'] == 0] > 0)
    os.environ['HMPC_JIT_SELFCHECK'] = '0'           # (no first-use check, no second opinion: what the compiled kernel itself returns)
    try:
        spec = HipBatchedQP(data)
        os.environ['HMPC_JIT'] = '0'
        try:
            gen = HipBatchedQP(data)
        finally:
            del os.environ['HMPC_JIT']
    finally:
        del os.environ['HMPC_JIT_SELFCHECK']
    assert spec.kernel_info() == (6, 6, 6) and gen.kernel_info() == (0, 0, 0)
    for waves in ('1', '2', '4'):
        os.environ['HMPC_WAVES'] = waves
        try:
            a, g = spec.solve_batch(x0, fix), gen.solve_batch(x0, fix)
        finally:
            del os.environ['HMPC_WAVES']
        for name, r in (('register kernel', a), ('run-time-sized kernel', g)):
            assert np.array_equal(r['status'], b['status']), (name, waves, np.flatnonzero(r['status'] != b['status']))
            assert np.all(r['polished'][r['status'] == 0] > 0), (name, waves, np.flatnonzero((r['status'] == 0) & (r['polished'] == 0)))
        _compare(ctrl, a, b, T, fix, min_polished=1.0, x0=x0, efloor=1e-5)
        _compare(ctrl, g, b, T, fix, min_polished=1.0, x0=x0, efloor=1e-5)
    assert spec.jit_stats() == (0, 0, 0)


def _undecided_by_design(monkeypatch):
    """A compiled kernel that leaves every fifth node NUMERICAL (test hook HMPC_TEST_UNDECIDED of hmpc_kernel.hip, through the flags
    of the run-time compilation: a cache entry of its own), with the first-use check skipped: what the SECOND net has to catch."""
    monkeypatch.setenv('HMPC_JIT_FLAGS', '-DHMPC_TEST_UNDECIDED=5')
    monkeypatch.setenv('HMPC_JIT_SELFCHECK_SKIP_FIRST', '1')


@pytest.mark.parametrize('entry', ['host', 'device', 'fleet'])
def test_a_compiled_kernel_that_leaves_nodes_undecided_gets_a_second_opinion(monkeypatch, capfd, entry):
    # The reference never hands back an undecided node (bounded_qp.py:216-228 asserts).  Kernels compiled at hmpc_create have
    # come out wrong from this compiler -- always loudly, nodes ending NUMERICAL --, so EVERY entry that solves
    # lists the nodes such a kernel leaves MAXITER / NUMERICAL on the device and has the shipped kernel solve them again in the
    # same stream (hmpc_solve_batch_device): the caller gets decided records whatever the compiled kernel did, and a compiled
    # kernel that leaves nodes undecided which the shipped one decides is dropped when the counts arrive.  Here the compiled
    # kernel is wrong BY DESIGN (every fifth node), the first-use check is skipped, and the three entries are walked.
    import torch
    ctrl_ok = make_controller('cart_pole_with_walls', T=10, backend='hip')
    x0 = np.array([0., 0., .5, 0.])
    fix = random_prefix_frontier(10, 4, 1500, p_one=0.1)
    fix[0, :] = -1
    ref = ctrl_ok.qp.solve_batch(x0, fix)
    assert np.all(ref['status'] <= 1) and ctrl_ok.qp.kernel_info() == (6, 6, 6)
    _undecided_by_design(monkeypatch)
    bad = make_controller('cart_pole_with_walls', T=10, backend='hip')
    assert bad.qp.kernel_info() == (6, 6, 6)
    capfd.readouterr()
    if entry == 'host':
        got = bad.qp.solve_batch(x0, fix)                                  # (1500 nodes: one wave per node)
        st, obj, prim = got['status'], got['obj'], got['primal']
    elif entry == 'device':
        dev = torch.device('cuda', 0)
        out = dict(obj=torch.empty(1500, dtype=torch.float64, device=dev), dual_obj=torch.empty(1500, dtype=torch.float64, device=dev),
                   status=torch.empty(1500, dtype=torch.int32, device=dev), iters=torch.empty(1500, dtype=torch.int32, device=dev),
                   primal=torch.empty(1500, bad.qp.n_primal, dtype=torch.float64, device=dev),
                   dual=torch.empty(1500, bad.qp.n_dual, dtype=torch.float64, device=dev))
        bad.qp.solve_batch_device(torch.from_numpy(x0).to(dev), torch.from_numpy(fix).to(dev), out)
        torch.cuda.synchronize()
        got = record_from_device(*(out[k].cpu().numpy() for k in ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual')))
        st, obj, prim = got['status'], got['obj'], got['primal']
    else:
        from warm_start_hmpc_amd.fleet import FleetMPC
        errors = load_fixture('reference_closed_loop')['errors_0003'][:3, :4]
        good = FleetMPC(ctrl_ok, 3).closed_loop(np.array([0., 0., .5, 0.]), 4, errors, frontier_width=8)
        st = None
        fl = FleetMPC(bad, 3).closed_loop(np.array([0., 0., .5, 0.]), 4, errors, frontier_width=8)   # (raises on a node that stays undecided)
        np.testing.assert_allclose(fl['costs'], good['costs'], rtol=1e-9, atol=1e-12)
        assert np.array_equal(fl['len_ws'], good['len_ws'])
    if st is not None:
        assert np.array_equal(st, ref['status']) and np.all(st <= 1)
        fin = st == 0
        np.testing.assert_allclose(obj[fin], ref['obj'][fin], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(prim[fin], ref['primal'][fin], rtol=0, atol=1e-7)
        # the batch mixes records of two kernels (every fifth node is the shipped kernel's): each certifies itself, at the base tolerances
        counts = assert_certified(bad, x0, fix, got, what='second opinion, %s entry' % entry)
        assert counts['skipped'] == 0 and counts['polished'] + counts['unpolished'] == fin.sum()
    dropped, runs, agreed = bad.qp.jit_stats()                              # (takes the counts of the last call in)
    err = capfd.readouterr().err
    assert dropped >= 1 and runs >= 1 and agreed == 0, (dropped, runs, agreed)
    assert 'undecided of which the shipped kernel decides' in err
    assert 2 in bad.qp.kernel_info()                                        # the shipped register kernel serves where it was dropped


def test_a_healthy_compiled_kernel_costs_its_second_opinion_nothing_but_two_empty_launches():
    # every default kernel: no node undecided, nothing dropped, the same records as without the nets (bitwise)
    x0 = np.array([0., 0., .5, 0.])
    fix = random_prefix_frontier(10, 4, 600, p_one=0.1)
    a = make_controller('cart_pole_with_walls', T=10, backend='hip')
    os.environ['HMPC_JIT_SELFCHECK'] = '0'
    try:
        b = make_controller('cart_pole_with_walls', T=10, backend='hip')
    finally:
        del os.environ['HMPC_JIT_SELFCHECK']
    ra, rb = a.qp.solve_batch(x0, fix), b.qp.solve_batch(x0, fix)
    for k in ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual'):
        assert np.array_equal(ra[k], rb[k], equal_nan=True), k
    assert a.qp.jit_stats() == (0, 1, 0) and b.qp.jit_stats() == (0, 0, 0)


def test_the_ilp_schedule_is_only_for_validated_binaries(monkeypatch):
    # The compiler's ILP schedule is worth 8 - 15 % and produced most of the wrong binaries of rounds 4 and 5 (one did not come back
    # from a launch): hmpc_create uses it only for binaries listed in the cache's VALIDATED manifest (csrc/hmpc_jit.h; written by
    # tests/gpu_validate_ilp.py), every other problem gets the compiler's default schedule.  The headline problem is in the
    # manifest the tree ships; a random MLD nobody has validated is not; both give the oracle's records.
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    from oracle.oracle_qp import OracleBatchedQP
    head = make_controller('cart_pole_with_walls', backend='hip')
    assert head.qp.kernel_info() == (6, 6, 6) and head.qp.kernel_recipe() == (1, 1, 1), (head.qp.kernel_info(), head.qp.kernel_recipe())
    monkeypatch.setenv('HMPC_JIT_SCHED', 'default')
    plain = make_controller('cart_pole_with_walls', backend='hip')
    monkeypatch.delenv('HMPC_JIT_SCHED')
    assert plain.qp.kernel_info() == (6, 6, 6) and plain.qp.kernel_recipe() == (0, 0, 0)
    fix = random_prefix_frontier(20, 4, 200, p_one=0.1)
    fix[0, :] = -1
    a, c = head.qp.solve_batch(X0, fix), plain.qp.solve_batch(X0, fix)
    assert np.array_equal(a['status'], c['status'])
    fin = a['status'] == 0
    np.testing.assert_allclose(a['obj'][fin], c['obj'][fin], rtol=1e-9, atol=1e-12)
    mld, objective, x0 = random_mld(nx=5, nuc=2, nub=2, seed=21)                      # (not among the problems of tests/jit_problems.py)
    ctrl = HybridModelPredictiveController(mld, 9, objective, None, backend=_NoBackend())
    new = HipBatchedQP(ctrl.problem_data())
    assert new.kernel_info() == (6, 6, 6) and new.kernel_recipe() == (0, 0, 0), (new.kernel_info(), new.kernel_recipe())
    f2 = random_prefix_frontier(9, 2, 128, p_one=0.3)
    f2[0, :] = -1
    _compare(ctrl, new.solve_batch(x0, f2), OracleBatchedQP(ctrl.problem_data(), threads=8).solve_batch(x0, f2), 9, f2, min_polished=0.99, x0=x0, efloor=1e-5)


def test_without_a_compiler_at_run_time_the_shipped_kernels_serve(monkeypatch, tmp_path):
    # hmpc_create compiles the kernels of a problem (csrc/hmpc_jit.h); a host without the compiler -- or without the sources, or
    # with an empty cache it cannot fill -- gets the shipped kernels: built-in register kernels for the cart-pole shapes, the
    # run-time-sized kernel for every other system.  Same records.
    from jit_problems import problem, REGISTER_SHAPES
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    x0 = np.array([0., 0., .5, 0.])
    fix = random_prefix_frontier(10, 4, 48, p_one=0.1)
    fix[0, :] = -1
    a = make_controller('cart_pole_with_walls', T=10, backend='hip')
    assert a.qp.kernel_info() == (6, 6, 6)
    monkeypatch.setenv('HMPC_HIPCC', '/nonexistent/hipcc')
    monkeypatch.setenv('HMPC_JIT_CACHE', str(tmp_path))
    b = make_controller('cart_pole_with_walls', T=10, backend='hip')
    assert b.qp.kernel_info() == (2, 2, 2), b.qp.kernel_info()
    ra, rb = a.qp.solve_batch(x0, fix), b.qp.solve_batch(x0, fix)
    assert np.array_equal(ra['status'], rb['status'])
    fin = ra['status'] == 0
    np.testing.assert_allclose(ra['obj'][fin], rb['obj'][fin], rtol=1e-9, atol=1e-12)
    data, mld, objective, xr = problem(*REGISTER_SHAPES[0])
    c = HipBatchedQP(data)
    assert c.kernel_info() == (0, 0, 0), c.kernel_info()
    assert os.listdir(tmp_path) == []


def test_two_launch_form_of_the_lazy_terminal_set(monkeypatch):
    # Opt-in (HMPC_SPLIT=1): large cold batches leave the nodes that need the terminal-set rows to a second launch (four
    # waves per node, each from its own first record: hmpc_capi.hip, DevWarm).  Same statuses and the same vertices as the
    # one-launch form and as the oracle; the nodes of real trees from closed-loop states: ~6 % of them take that path.
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import real_tree_frontier
    hip = make_controller('cart_pole_with_walls', backend='hip')
    x0, fix, _ = real_tree_frontier(hip, 2048, 0, load_fixture('cart_pole_with_walls')['x_max'], spread=0.05)
    monkeypatch.setenv('HMPC_SPLIT', '1')            # (opt-in: measured slower than the one-launch form, hmpc_capi.hip)
    a = hip.qp.solve_batch(x0, fix)
    monkeypatch.delenv('HMPC_SPLIT')
    b = hip.qp.solve_batch(x0, fix)
    assert hip.qp.launch_info()[0] >= 1024                                # (one wave per node: the form that splits)
    assert 20 <= a['second'].sum() <= 400 and b['second'].sum() == 0   # (the one-launch cold kernel does not raise the flag)
    assert np.array_equal(a['status'], b['status']) and np.all(a['status'] <= 1)
    fin = a['status'] == 0
    assert np.all(a['polished'][fin] > 0) and np.all(b['polished'][fin] > 0)
    np.testing.assert_allclose(a['obj'][fin], b['obj'][fin], rtol=1e-9, atol=1e-12)
    xs = 21 * 4
    dev = np.max(np.abs(a['primal'][fin][:, :xs] - b['primal'][fin][:, :xs]), axis=1) / np.maximum(1e-2, np.max(np.abs(b['primal'][fin][:, :xs]), axis=1))
    assert dev.max() < 1e-7, dev.max()
    differ = int((a['iters'] != b['iters']).sum())                          # (the second solves: fewer iterations from the first record)
    assert 20 <= differ <= 400 and a['iters'][a['iters'] != b['iters']].mean() < b['iters'][a['iters'] != b['iters']].mean()
    inf = a['status'] == 1
    np.testing.assert_allclose(a['dual'][inf], b['dual'][inf], rtol=0, atol=1e-6)
    orc = make_controller('cart_pole_with_walls', backend='oracle', threads=8)
    sub = np.flatnonzero(a['iters'] != b['iters'])[:64]
    sub = np.concatenate((sub, np.arange(64)))
    _compare(hip, {k: v[sub] for k, v in a.items() if isinstance(v, np.ndarray) and v.shape[:1] == (len(fix),)},
             orc.qp.solve_batch(x0[sub], fix[sub]), 20, fix[sub], x0=x0[sub])


@pytest.mark.parametrize('waves', ['1', '2', '4'])
def test_a_node_on_the_boundary_between_feasible_and_infeasible_is_decided(monkeypatch, waves):
    # tests/golden/hard_node_sd003.npz: met when the published sd = .003 runs are replayed with cold searches only (no
    # hand-down: the reference's setting).  tau collapses while NO ray verifies -- f'y + h'z and E'y + C'z both go to zero,
    # eta changes sign from one iteration to the next: the node is infeasible by less than the accuracy of the arithmetic.
    # Until round 4 the kernel ran it to 100 iterations, twice, and could end MAXITER (the study stopped on it); the oracle
    # leaves at iteration 37 with a ray that happens to verify.  Now: infeasible on both sides, the kernel's ray flagged
    # WEAK (pruned at this step, never carried to the next), decided within ~40 iterations.
    d = load_fixture('hard_node_sd003')
    hip = make_controller('cart_pole_with_walls', backend='hip')
    orc = make_controller('cart_pole_with_walls', backend='oracle')
    monkeypatch.setenv('HMPC_WAVES', waves)
    a = hip.qp.solve_batch(d['x0'][0], d['fix'])
    monkeypatch.delenv('HMPC_WAVES')
    b = orc.qp.solve_batch(d['x0'][0], d['fix'])
    assert a['status'][0] == 1 and b['status'][0] == 1
    # (which side's ray happens to verify on this node is a matter of its rounding: until the end-game fraction of round 5 the
    # oracle's did and the kernel's was WEAK, since then the other way round at one wave per node.  A side that does not flag its
    # ray WEAK has checked it: residual <= 1e-6 eta, eta > 0 -- a positive dual objective.)
    assert a['iters'][0] <= 60
    for r in (a, b):
        assert r['weak'][0] == 1 or r['dual_obj'][0] > 0


def test_streaming_kernel_baseline_config4():
    # BASELINE.json configs[4] (random MLD nx=20, nu=6+8, N=30; rows as in SURVEY 8(d) C4): lists and
    # Riccati factor do not fit one CU's LDS, the generic kernel's streaming form keeps them in global memory
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    from oracle.oracle_qp import OracleBatchedQP
    mld, objective, x0 = random_mld()
    T = 30
    ctrl = HybridModelPredictiveController(mld, T, objective, None, backend=_NoBackend())
    hip, orc = HipBatchedQP(ctrl.problem_data()), OracleBatchedQP(ctrl.problem_data(), threads=8)
    # frontier: prefixes of a dive to a feasible leaf (binaries of stage t from the sign of c_j'x_t of the
    # current relaxation), every other one with one flipped binary -- random prefixes are all infeasible here
    nub, nx = 8, 20
    leaf = dive_leaf(orc, mld, x0, T, feasible=True)
    # BASELINE's size: the 4096 DISTINCT nodes of the bench's dive frontier (bench.dive_frontier; until round 3: 256 nodes)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import dive_frontier
    fix = dive_frontier(leaf, 4096, 0)
    orc.threads = os.cpu_count() or 8
    a, b = hip.solve_batch(x0, fix), orc.solve_batch(x0, fix)
    assert hip.launch_info()[1] > 100 * 1024          # the streaming carve: vectors only, still most of a CU
    # round 4: the kernel that runs is the streaming form COMPILED WITH THIS PROBLEM'S SIZES (csrc/hmpc_jit.h; four waves per
    # node, the only wave count that form runs); the shipped run-time-sized build (HMPC_JIT_SIZED=0) returns the same records
    assert hip.kernel_info() == (1, 1, 5), hip.kernel_info()
    os.environ['HMPC_JIT_SIZED'] = '0'
    try:
        plain = HipBatchedQP(ctrl.problem_data())
    finally:
        del os.environ['HMPC_JIT_SIZED']
    assert plain.kernel_info() == (1, 1, 1)
    c = plain.solve_batch(x0, fix[:512])
    assert np.array_equal(c['status'], a['status'][:512]) and np.array_equal(c['polished'] > 0, a['polished'][:512] > 0)
    fin = c['status'] == 0
    np.testing.assert_allclose(c['obj'][fin], a['obj'][:512][fin], rtol=1e-9, atol=1e-12)
    assert np.max(np.abs(c['primal'][fin][:, :(T + 1) * nx] - a['primal'][:512][fin][:, :(T + 1) * nx])) < 1e-8
    # this generator leaves the binaries out of the cost (R = [I 0], as the reference does): states and continuous
    # inputs are unique and compared at RTOL like everywhere else, the relaxed binaries are not.  Every record at the one
    # tolerance; >= 99 % of the optimal nodes polished (measured: all of them, on both sides -- the tolerance escalation
    # of round 4; until then 2 % returned an iterate 1e-4 off); a seeded sample of the kernel's polished records against
    # the dense active-set solve, which shares no code with kernel or oracle.
    # (element-wise floor 1e-5 here: the states of this system decay to 1e-7 along the horizon, and a vertex computed by the
    # method of multipliers at rho = 1e5 is good to ~1e-11 absolute -- measured worst 3.5e-11 on a component of 1e-7 among
    # 3631 x 620 -- which is 1e-5 of a component of 1e-6; norm-wise the worst deviation is 3.7e-8)
    _compare(ctrl, a, b, T, fix, min_polished=0.99, x0=x0, efloor=1e-5)
    # a record that is NOT polished certifies itself (no reference involved): feasible, dual feasible, duality gap
    for i in np.flatnonzero((a['status'] == 0) & (a['polished'] == 0)):
        sol = SubproblemSolution.from_rows(ctrl.layout, fix[i], a['obj'][i], a['dual_obj'][i], a['status'][i], a['primal'][i], a['dual'][i])
        ident = {(k // nub, k % nub): float(v) for k, v in enumerate(fix[i]) if v >= 0}
        assert check_solution(ctrl, sol, ident, x0, tol=5e-6) == 'optimal'
    assert (a['status'] == 0).sum() >= 1 and (a['status'] == 1).sum() >= 1
    # a problem whose vectors alone exceed a CU's LDS is still refused loudly
    huge = HybridModelPredictiveController(mld, 60, objective, None, backend=_NoBackend())
    with pytest.raises(RuntimeError, match='LDS'):
        HipBatchedQP(huge.problem_data())


@pytest.mark.parametrize('nx,nuc,nub,T,seed', [(13, 3, 5, 12, 1), (8, 8, 8, 10, 3), (32, 10, 8, 6, 10), (16, 4, 0, 8, 8)])
def test_streaming_kernel_other_shapes(monkeypatch, nx, nuc, nub, T, seed):
    # the streaming form forced onto other random MLDs: a state count that is no multiple of four (padded blocks, partial
    # batches of the matrix-core tiles), nu = 16 (the limit of the panel form), nz = 50 with nu = 18 (the LDS form of the
    # factorisation), no binaries at all -- tests/gpu_streaming_shapes.py runs twelve of them on the bounds-checked build
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    from oracle.oracle_qp import OracleBatchedQP
    mld, objective, x0 = random_mld(nx=nx, nuc=nuc, nub=nub, seed=seed)
    ctrl = HybridModelPredictiveController(mld, T, objective, None, backend=_NoBackend())
    monkeypatch.setenv('HMPC_FORCE_BIG', '1')
    hip = HipBatchedQP(ctrl.problem_data())
    monkeypatch.delenv('HMPC_FORCE_BIG')
    orc = OracleBatchedQP(ctrl.problem_data(), threads=8)
    count = 48
    fix = np.full((count, T * nub), -1, np.int8)
    if nub:
        leaf = dive_leaf(orc, mld, x0, T, feasible=True)[None]
        rng = np.random.default_rng(seed)
        for k in range(1, count):
            d = int(rng.integers(1, T * nub + 1))
            fix[k, :d] = leaf[0, :d]
            if k % 2 == 0:
                j = int(rng.integers(0, d))
                fix[k, j] = 1 - fix[k, j]
    a, b = hip.solve_batch(x0, fix), orc.solve_batch(x0, fix)
    assert hip.launch_info()[0] >= 1
    _compare(ctrl, a, b, T, fix, min_polished=0.99, x0=x0, efloor=1e-5)
    assert (a['status'] == 0).sum() >= 1


def test_streaming_kernel_forced_on_cart_pole(monkeypatch):
    # the same streaming code path on the reference's system, against the oracle
    monkeypatch.setenv('HMPC_FORCE_BIG', '1')
    hip = make_controller('cart_pole_with_walls', backend='hip')
    monkeypatch.delenv('HMPC_FORCE_BIG')
    orc = make_controller('cart_pole_with_walls', backend='oracle', threads=8)
    fix = random_prefix_frontier(20, 4, 96, p_one=0.2, seed0=7000)
    fix[0, :] = -1
    _compare(hip, hip.qp.solve_batch(X0, fix), orc.qp.solve_batch(X0, fix), 20, fix, x0=X0)


def test_lockstep_closed_loops_on_gpu():
    # many closed loops in lockstep; the GPU walk must be the oracle's walk
    from warm_start_hmpc_amd.batched import BatchedMPC
    x_max = load_fixture('cart_pole_with_walls')['x_max']
    runs = {}
    for name in ('hip', 'oracle'):
        ctrl = make_controller('cart_pole_with_walls', backend=name, **({'threads': 8} if name == 'oracle' else {}))
        runs[name] = BatchedMPC(ctrl).closed_loop(X0, n_steps=4, e_sd=0.003, seeds=(0, 1, 2, 3), x_max=x_max,
                                                  frontier_width=8, cold_too=True)
    a, b = runs['hip'], runs['oracle']
    assert a['steps'] == b['steps'] == 16
    for k in range(4):
        np.testing.assert_allclose(a['costs'][k], b['costs'][k], rtol=1e-6)
        assert a['len_ws'][k][0] == 77
        assert max(a['nodes_ws'][k][1:]) <= 60 and min(a['nodes_cs'][k]) >= 150


def _shift_copied(ctrl):
    """Columns of a shifted dual row that are copies or zeros: everything but mu'_{T-2} and rho'_{T-1} (tests/test_shift.py
    holds those two to an extended-precision reference)."""
    cut, T = ctrl.layout.dual_slices(), ctrl.T
    copied = np.ones(ctrl.layout.n_dual, dtype=bool)
    copied[cut['mu'][T - 2]] = False
    copied[cut['rho'][T - 1]] = False
    return copied


def test_device_warm_start_shift_matches_host_forms():
    # the node shift of controller.py:431-721 as one kernel launch over the leaves of
    # several trees, against (a) the vectorised numpy form and (b) the reference-shaped per-leaf Python form
    from warm_start_hmpc_amd.batched import BatchedMPC
    ctrl = make_controller('cart_pole_with_walls', backend='hip')
    bm = BatchedMPC(ctrl)
    assert bm.device_shift
    x_max = load_fixture('cart_pole_with_walls')['x_max']
    rng = np.random.RandomState(3)
    x0s = np.array([X0, X0 * 0.8, X0 * 0.9])
    res = bm.feedforward_many(x0s, None, frontier_width=8)
    e0s = 0.01 * rng.randn(3, 4) * x_max                       # large enough to reopen some infeasible leaves
    u0s = np.array([np.concatenate((r['uc'][0], r['ub'][0])) for r in res])
    dev = bm.construct_warm_start_many([r['leaves'] for r in res], x0s, u0s, e0s)
    reopened = 0
    for k, r in enumerate(res):
        ref = bm.construct_warm_start(r['leaves'], x0s[k], r['uc'][0], r['ub'][0], e0s[k])
        d = dev[k]
        assert len(d) == len(ref) == 77 or len(d) == len(ref)
        assert np.array_equal(d.fix, ref.fix)
        assert np.array_equal(np.isinf(d.lb), np.isinf(ref.lb))
        fin = np.isfinite(ref.lb)
        np.testing.assert_allclose(d.lb[fin], ref.lb[fin], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(d.dual, ref.dual, rtol=1e-12, atol=1e-13)
        np.testing.assert_array_equal(d.dual[:, _shift_copied(ctrl)], ref.dual[:, _shift_copied(ctrl)])   # copies and zeros: exact
        np.testing.assert_allclose(d.dobj, ref.dobj, rtol=1e-10, atol=1e-12)
        assert np.array_equal(d.has_dual, ref.has_dual)
        reopened += int((~d.has_dual).sum())
    # (b) one tree through the reference-shaped API: same cover, same bounds
    sol, leaves, _, _ = ctrl.feedforward(x0s[0], printing_period=None, frontier_width=8)
    ws = ctrl.construct_warm_start(leaves, x0s[0], sol.variables['uc'][0], sol.variables['ub'][0], e0s[0])[0]
    lb_api = sorted(float(n.lb) for n in ws)
    lb_dev = sorted(float(v) for v in dev[0].lb)
    assert len(lb_api) == len(lb_dev)
    np.testing.assert_allclose(lb_dev, lb_api, rtol=1e-8, atol=1e-10)
    # and the shifted trees drive the next step to the same optimum as a cold start
    x1 = np.array([r['x'][1] for r in res]) + e0s
    warm = bm.feedforward_many(x1, dev, frontier_width=8)
    cold = bm.feedforward_many(x1, None, frontier_width=8)
    for w, c in zip(warm, cold):
        assert np.isclose(w['objective'], c['objective'], rtol=1e-5, atol=1e-8) or (np.isinf(w['objective']) and np.isinf(c['objective']))
        assert w['solves'] < c['solves']


@pytest.mark.parametrize('rows', ['1', '0'])
@pytest.mark.parametrize('fixture,T', [('cart_pole_with_walls', 5), ('cart_pole_one_wall', 8), ('cart_pole_with_walls', 40)])
def test_both_shift_kernels_on_odd_shapes(monkeypatch, fixture, T, rows):
    # csrc/hmpc_shift.hip holds two kernels: rows staged in LDS by the memory pipeline (HMPC_SHIFT_ROWS unset / 1) and rows through
    # registers (0; what long rows get).  Shapes the headline problem does not have: an ODD row length (with_walls N = 5: 335
    # entries -- 8-byte stores, the last entry fetched by itself), odd counts of rows and columns of M_mu (one_wall: 19 x 27 -- a
    # column paired with zeros), rows of 16 KB (N = 40: seven waves per CU).  Both against the per-leaf host form.
    from warm_start_hmpc_amd.batched import BatchedMPC
    monkeypatch.setenv('HMPC_SHIFT_ROWS', rows)
    ctrl = make_controller(fixture, T=T, backend='hip')
    assert ctrl.qp.n_dual % 2 == (1 if (fixture, T) == ('cart_pole_with_walls', 5) else 0)
    bm = BatchedMPC(ctrl)
    assert bm.device_shift
    x_max = load_fixture(fixture)['x_max']
    rng = np.random.RandomState(5)
    x0s = np.array([X0 * 0.5, X0 * 0.3])
    res = bm.feedforward_many(x0s, None, frontier_width=8)
    assert all(np.isfinite(r['objective']) for r in res)
    e0s = 0.01 * rng.randn(2, 4) * x_max
    u0s = np.array([np.concatenate((r['uc'][0], r['ub'][0])) for r in res])
    dev = bm.construct_warm_start_many([r['leaves'] for r in res], x0s, u0s, e0s)
    for k, r in enumerate(res):
        ref = bm.construct_warm_start(r['leaves'], x0s[k], r['uc'][0], r['ub'][0], e0s[k])
        d = dev[k]
        assert len(d) == len(ref) > 0
        assert np.array_equal(d.fix, ref.fix)
        assert np.array_equal(np.isinf(d.lb), np.isinf(ref.lb))
        fin = np.isfinite(ref.lb)
        np.testing.assert_allclose(d.lb[fin], ref.lb[fin], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(d.dual, ref.dual, rtol=1e-12, atol=1e-13)
        np.testing.assert_array_equal(d.dual[:, _shift_copied(ctrl)], ref.dual[:, _shift_copied(ctrl)])   # copies and zeros: exact
        np.testing.assert_allclose(d.dobj, ref.dobj, rtol=1e-10, atol=1e-12)
        assert np.array_equal(d.has_dual, ref.has_dual)


def test_warm_start_properties_on_gpu():
    # The reference's warm-start properties (warm_start_hmpc/test/test_controller.py:122-163) on the HIP backend: leaves
    # produced by the kernel, shifted (a) by the host form behind construct_warm_start and (b) by hmpc_shift_kernel;
    # checked through the reference's checkers restated in kkt_checks.py, not through the oracle:
    #   implied lower bounds <= the optimum of the node at the next state; shifted multipliers dual feasible
    #   (stationarity 1e-5 relative, signs); dual objective of a shifted multiplier == node.lb (1e-6) for finite bounds,
    #   > 0 for shifted infeasibility proofs; warm == cold cost.
    from kkt_checks import dual_residuals, dual_objective
    from warm_start_hmpc_amd.batched import BatchedMPC
    from warm_start_hmpc_amd.subproblem_solution import DualSolution
    hip = make_controller('cart_pole_with_walls', backend='hip')
    sol, leaves, solves, _ = hip.feedforward(X0, printing_period=None)
    np.random.seed(1)
    uc0, ub0 = sol.variables['uc'][0], sol.variables['ub'][0]
    e0 = np.random.randn(hip.mld.nx) * .001
    x1 = hip.mld.A.dot(X0) + hip.mld.B.dot(np.concatenate((uc0, ub0))) + e0
    ws = hip.construct_warm_start(leaves, X0, uc0, ub0, e0)[0]
    assert len(ws) == 77 and is_disjoint_cover(hip, ws)         # published cover size (solve_log_sd_0.000.log:8)
    # the nodes of the cover at the next state, one launch
    fix = np.array([hip._fix_vector(n.identifier) for n in ws], dtype=np.int8)
    at_x1 = hip.qp.solve_batch(x1, fix)
    assert np.all(at_x1['status'] <= 1)

    def properties(identifier, lb, variables, x):
        zero, nonneg = dual_residuals(hip, variables)
        assert np.max(np.abs(zero)) < 1e-5 * (1 + np.max(np.abs(np.concatenate(variables['mu']))))
        assert np.min(nonneg) >= -1e-9
        obj = max(0., dual_objective(hip, variables, identifier, x))
        if np.isinf(lb):
            assert obj > 0.
            return 1
        assert abs(obj - lb) < 1e-6
        return 0
    kept = 0
    for k, node in enumerate(ws):
        assert at_x1['obj'][k] >= node.lb - 1e-7                # implied bounds are valid (inf: the node IS infeasible)
        if node.extra.dual is not None:
            kept += properties(node.identifier, node.lb, node.extra.dual.variables, x1)
    assert kept >= 70                                           # the Farkas proofs survive the shift (73-75 of 77)
    # (b) the same leaves through the shift kernel
    bm = BatchedMPC(hip)
    assert bm.device_shift
    res = bm.feedforward_many(X0[None], None, frontier_width=1)
    r = res[0]
    u0 = np.concatenate((r['uc'][0], r['ub'][0]))
    assert np.array_equal(np.round(r['ub'][0]), np.round(ub0))
    dev = bm.construct_warm_start_many([r['leaves']], X0[None], u0[None], e0[None])[0]
    x1d = hip.mld.A.dot(X0) + hip.mld.B.dot(u0) + e0
    assert len(dev) == 77
    at_x1d = hip.qp.solve_batch(x1d, dev.fix)
    kept = 0
    for k in range(len(dev)):
        assert at_x1d['obj'][k] >= dev.lb[k] - 1e-7
        if dev.has_dual[k]:
            d = DualSolution.from_row(hip.layout, dev.dobj[k], dev.dual[k])
            ident = {(q // hip.mld.nub, q % hip.mld.nub): float(v) for q, v in enumerate(dev.fix[k]) if v >= 0}
            kept += properties(ident, dev.lb[k], d.variables, x1d)
    assert kept >= 70
    cold = hip.feedforward(x1d, printing_period=None)
    warm = hip.feedforward(x1d, printing_period=None, warm_start=ws)
    assert warm[0].objective == cold[0].objective               # test_controller.py:165-170 (assertEqual)
    assert warm[2] <= 25 and cold[2] >= 150                     # published: 10-17 warm, 158-161 cold


def test_replayed_real_frontier():
    # SURVEY 8(d) C2, second frontier: every node a cold-started branch and bound actually solved (about 160)
    # plus its 81 leaves, tiled to 1024 nodes and solved in one launch
    orc = make_controller('cart_pole_with_walls', backend='oracle', threads=8)
    seen = []
    inner = orc.solve_frontier

    def recording(identifiers, x0):
        seen.extend(orc._fix_vector(i) for i in identifiers)
        return inner(identifiers, x0)
    orc.solve_frontier = recording
    sol, leaves, solves, _ = orc.feedforward(X0, printing_period=None)
    orc.solve_frontier = inner
    assert len(seen) == solves and len(leaves) == 81
    nodes = np.array(seen + [orc._fix_vector(l.identifier) for l in leaves], dtype=np.int8)
    fix = np.tile(nodes, (1024 // len(nodes) + 1, 1))[:1024]
    hip = make_controller('cart_pole_with_walls', backend='hip')
    a, b = hip.qp.solve_batch(X0, fix), orc.qp.solve_batch(X0, fix)
    _compare(hip, a, b, 20, fix, x0=X0)
    feasible = (a['status'] == 0).mean()
    assert 0.3 < feasible < 0.7                                        # about half of a real tree's nodes are feasible
    # copies of the same node in different batch positions give the same bits
    assert np.array_equal(a['obj'][:len(nodes)], a['obj'][len(nodes):2 * len(nodes)], equal_nan=True)
    # the incumbent of the search is the best fully fixed node of the frontier
    full = (fix >= 0).all(axis=1) & (a['status'] == 0)
    assert abs(a['obj'][full].min() - sol.objective) <= 1e-8 * (1 + sol.objective)


def test_replay_frontier_at_n40_as_the_bench_times_it():
    # BASELINE configs[3] at the size the bench times it: the replay frontier of ITS OWN tree -- the
    # 320 nodes a cold-started search from x0 = [0, 0, 1, 0] solves at N = 40 plus its 161 leaves, bench.real_tree_frontier, untiled
    # (481 nodes; the bench tiles them to 2048) -- against the oracle at the one tolerance, every polished record against the dense
    # active-set solve; solved as one batch (two waves per node) and with one / four waves per node.
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import real_tree_frontier
    hip = make_controller('cart_pole_with_walls', T=40, backend='hip')
    orc = make_controller('cart_pole_with_walls', T=40, backend='oracle', threads=16)
    x0, fix, parent = real_tree_frontier(hip, 2048, 0, None, spread=0.)
    count = int(np.flatnonzero(parent[1:] == -1)[0]) + 1 if np.any(parent[1:] == -1) else len(fix)   # (the tiling starts over at the second root)
    assert 470 <= count <= 490, count
    x0, fix = x0[:count], fix[:count]
    b = orc.qp.solve_batch(x0, fix)
    assert 0.25 < (b['status'] == 0).mean() < 0.6
    for waves in (None, '1', '4'):
        if waves:
            os.environ['HMPC_WAVES'] = waves
        try:
            a = hip.qp.solve_batch(x0, fix)
        finally:
            os.environ.pop('HMPC_WAVES', None)
        _compare(hip, a, b, 40, fix, x0=x0)
    assert hip.qp.jit_stats()[0] == 0


def test_bounded_qp_accessors_on_gpu():
    # the reference's BoundedQP method set (bounded_qp.py:127-341) over the HIP backend, with the
    # identities of test_bounded_qp.py:104-189 (Farkas signs, dual objective = -sum rhs * multiplier, strong duality)
    exercise_bounded_qp(make_controller('cart_pole_with_walls', T=10, backend='hip'))


def test_speculative_expansion_on_gpu():
    # SURVEY 8(f) rank 3 on the HIP path: descendants ride in the launch of their ancestor; the search consumes the
    # same results in the same order (incumbent, leaves, bounds, solve count), in fewer launches
    import copy
    ctrl = make_controller('cart_pole_with_walls', backend='hip')
    base_stats, spec_stats = {}, {}
    sol0, leaves0, solves0, _ = ctrl.feedforward(X0, printing_period=None, stats=base_stats)
    sol1, leaves1, solves1, _ = ctrl.feedforward(X0, printing_period=None, speculation_depth=4, stats=spec_stats)
    assert solves0 == solves1 and len(leaves0) == len(leaves1) == 81
    assert [sorted(l.identifier.items()) for l in leaves0] == [sorted(l.identifier.items()) for l in leaves1]
    assert sol0.objective == sol1.objective
    assert np.array_equal(np.array(sol0.variables['ub']), np.array(sol1.variables['ub']))
    np.testing.assert_allclose([l.lb for l in leaves0], [l.lb for l in leaves1], rtol=1e-9, atol=1e-12)
    assert base_stats['rounds'] == solves0 and base_stats['speculative'] == 0
    assert spec_stats['rounds'] < solves0 // 3
    assert spec_stats['launched'] >= solves1 and spec_stats['wasted'] == spec_stats['launched'] - solves1
    ws = ctrl.construct_warm_start(leaves0, X0, sol0.variables['uc'][0], sol0.variables['ub'][0], np.zeros(4))[0]
    x1 = sol0.variables['x'][1]
    a_stats, b_stats = {}, {}
    sa = ctrl.feedforward(x1, warm_start=copy.deepcopy(ws), printing_period=None, stats=a_stats)
    sb = ctrl.feedforward(x1, warm_start=copy.deepcopy(ws), printing_period=None, speculation_depth=4, stats=b_stats)
    assert sa[2] == sb[2] and sa[0].objective == sb[0].objective
    assert b_stats['rounds'] < a_stats['rounds'] and b_stats['rounds'] <= 3


def test_feedback_closed_loop_on_gpu():
    # north_star names feedback(): five closed-loop steps on the HIP path walk the oracle's walk
    hip = make_controller('cart_pole_with_walls', backend='hip')
    orc = make_controller('cart_pole_with_walls', backend='oracle', threads=8)
    rng = np.random.RandomState(4)
    x_max = load_fixture('cart_pole_with_walls')['x_max']
    xh = xo = X0
    wh = wo = None
    for step in range(5):
        e0 = 0.003 * rng.randn(4) * x_max
        uh, wh, ih = hip.feedback(xh, warm_start=wh, e0=e0, speculation_depth=4)
        uo, wo, io = orc.feedback(xo, warm_start=wo, e0=e0)
        assert np.array_equal(uh[3:], uo[3:])                                    # applied binaries bit-exact
        assert _rel(uh[None, :3], uo[None, :3]).max() < RTOL
        assert _rel(ih['x1'][None], io['x1'][None]).max() < RTOL
        assert abs(ih['solution'].objective - io['solution'].objective) <= 1e-8 * (1 + io['solution'].objective)
        assert len(wh) == len(wo)
        if step:
            assert ih['qp_solves'] <= 60
        xh, xo = ih['x1'], io['x1']
