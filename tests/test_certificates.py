"""tests/certificates.py kept honest, without a GPU: (1) the oracle's records certify themselves at the base tolerances on the
workloads the GPU tests run -- which is what makes the bounds of the GPU tests a comparison with the reference and not with
the code under test --, (2) defects a kernel's write-out could have are caught, and were NOT caught by the comparison with the
oracle that the GPU tests made until now, (3) records land in the right class."""
import os
import sys

import numpy as np
import pytest

from helpers import make_controller, random_prefix_frontier, random_mld, real_tree_with_parents, dive_leaf, dive_and_prefix_frontier, _NoBackend
from certificates import assert_certified, residuals, classify, worst_per_class, BASE, OPTIMAL, RAY
from warm_start_hmpc_amd.controller import HybridModelPredictiveController
from oracle.oracle_qp import OracleBatchedQP

X0 = np.array([0., 0., 1., 0.])
MLDS = ((6, 2, 3, 8, 3), (8, 3, 4, 10, 2), (9, 3, 4, 6, 23), (8, 4, 4, 6, 23), (3, 3, 6, 12, 38))   # (nx, nuc, nub, T, seed): test_register_kernel_compiled_for_an_arbitrary_shape


def _random_mld_workload(nx, nuc, nub, T, seed):
    mld, objective, x0 = random_mld(nx=nx, nuc=nuc, nub=nub, seed=seed)
    ctrl = HybridModelPredictiveController(mld, T, objective, None, backend=_NoBackend())
    ctrl.qp = OracleBatchedQP(ctrl.problem_data(), threads=8)
    fix = dive_and_prefix_frontier(ctrl.qp, mld, x0, T, seed) if nub else np.full((4, 0), -1, np.int8)
    return ctrl, x0, fix


def _config4_workload(count=512):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import dive_frontier
    mld, objective, x0 = random_mld()
    T = 30
    ctrl = HybridModelPredictiveController(mld, T, objective, None, backend=_NoBackend())
    ctrl.qp = OracleBatchedQP(ctrl.problem_data(), threads=min(16, os.cpu_count() or 1))
    leaf = dive_leaf(ctrl.qp, mld, x0, T, feasible=True)                 # (the dive of test_streaming_kernel_baseline_config4)
    return ctrl, x0, dive_frontier(leaf, 4096, 0)[:count]


@pytest.mark.parametrize('fixture,T,terminal,count,p_one', [
    ('cart_pole_with_walls', 10, False, 64, 0.1),
    ('cart_pole_with_walls', 20, True, 256, 0.1),
    ('cart_pole_with_walls', 40, True, 48, 0.05),
    ('cart_pole_one_wall', 40, True, 96, 0.1),
])
def test_the_reference_certifies_on_random_prefixes(fixture, T, terminal, count, p_one):
    orc = make_controller(fixture, T=T, terminal=terminal, backend='oracle', threads=8)
    fix = random_prefix_frontier(T, orc.mld.nub, count, p_one=p_one)
    fix[0, :] = -1
    counts = assert_certified(orc, X0, fix, orc.qp.solve_batch(X0, fix), what=fixture)
    assert counts['polished'] >= 5 and counts['infeasible'] >= 40 and counts['weak'] == counts['skipped'] == counts['unpolished'] == 0


def test_the_reference_certifies_with_one_initial_state_per_node():
    orc = make_controller('cart_pole_with_walls', T=10, backend='oracle', threads=8)
    fix = random_prefix_frontier(10, 4, 96, p_one=0.05)                  # (the workload of test_per_node_initial_states)
    x0 = np.random.default_rng(5).uniform(-1, 1, (96, 4)) * np.array([.3, .1, .6, .4])
    counts = assert_certified(orc, x0, fix, orc.qp.solve_batch(x0, fix))
    assert counts['polished'] >= 10 and counts['infeasible'] >= 10 and counts['weak'] == counts['skipped'] == 0


@pytest.mark.parametrize('nx,nuc,nub,T,seed', MLDS + ((16, 4, 0, 8, 8),))      # (the last: no binaries at all, test_streaming_kernel_other_shapes)
def test_the_reference_certifies_on_random_mlds(nx, nuc, nub, T, seed):
    ctrl, x0, fix = _random_mld_workload(nx, nuc, nub, T, seed)
    counts = assert_certified(ctrl, x0, fix, ctrl.qp.solve_batch(x0, fix))
    assert counts['weak'] == counts['skipped'] == 0 and counts['polished'] >= (20 if nub else 4)


def test_the_reference_certifies_on_config4():
    ctrl, x0, fix = _config4_workload()
    counts = assert_certified(ctrl, x0, fix, ctrl.qp.solve_batch(x0, fix))
    assert counts['polished'] >= 400 and counts['infeasible'] >= 10 and counts['weak'] == counts['skipped'] == 0


def _vertex_guarantee(ctrl, rec, i):
    """What the polish GUARANTEES of a record it verified, in the units of the residuals (oracle/hsde_qp.c polish(), the same in
    hmpc_kernel.hip): rows are scaled to unit norm; an INACTIVE row may be violated by es = 1e-9 (1 + |w|_inf),
    an ACTIVE row is met to 1e-10 (1 + |w|_inf) at the second penalty level -- which enters the duality gap with its multiplier."""
    T, cut = ctrl.T, ctrl.layout.dual_slices()
    norms = [np.linalg.norm(np.hstack((ctrl.mld.F, ctrl.mld.G)), axis=1)] * (T - 1) + [np.linalg.norm(np.hstack((ctrl.F_Tm1, ctrl.G_Tm1)), axis=1)]
    winf = 1. + np.max(np.abs(rec['primal'][i]))
    weighted = sum(rec['dual'][i][cut['mu'][t]].dot(norms[t]) for t in range(T))
    return {'primal_inequality': 1e-9 * winf * max(n.max() for n in norms), 'gap': 1e-10 * winf * weighted / (1. + abs(rec['obj'][i]))}


@pytest.mark.parametrize('fixture,T', [('cart_pole_with_walls', 20), ('cart_pole_with_walls', 40), ('cart_pole_one_wall', 40)])
def test_the_reference_certifies_on_real_trees_cold_and_handed_down(fixture, T):
    orc = make_controller(fixture, T=T, backend='oracle', threads=8)
    fix, parent = real_tree_with_parents(orc, X0)
    cold = orc.qp.solve_batch(X0, fix)
    ok = (parent >= 0) & (cold['status'][np.maximum(parent, 0)] == 0) & (cold['polished'][np.maximum(parent, 0)] > 0)
    index = np.where(ok, parent, -1).astype(np.int32)
    warm = orc.qp.solve_batch(X0, fix, warm=(cold['primal'], cold['dual'], index))
    assert (warm['polished'] == 64).sum() >= 20                          # (verified hand-downs: they are in the polished class)
    # Two classes lie over the base of 1e-8, both by an inactive row of norm 51 / 273 that the polish verified on its UNIT form:
    #   with walls N = 40, handed down: primal inequality 1.5e-8 (2.9e-10 of the unit row) -- guaranteed: 7.2e-7
    #   one wall N = 40, cold and handed down (a node solved twice for the terminal set): primal inequality 1.1e-7 (4.0e-10 of
    #   the unit row) -- guaranteed: 1.0e-5; duality gap 1.9e-7 -- guaranteed: 4.0e-6
    # They are held, record by record, to what the polish guarantees (_vertex_guarantee) AND to a pin of 4 x the value measured (the
    # factor the GPU tests allow a kernel beside the oracle: a drift of the reference itself is seen here before it widens their
    # bound); every other residual of every class to its base.
    over = {('cart_pole_with_walls', 40, 'handed down'): {'primal_inequality': 4 * 1.5e-8},
            ('cart_pole_one_wall', 40, 'cold'): {'primal_inequality': 4 * 1.1e-7, 'gap': 4 * 1.9e-7},
            ('cart_pole_one_wall', 40, 'handed down'): {'primal_inequality': 4 * 1.1e-7, 'gap': 4 * 1.9e-7}}
    for what, rec in (('cold', cold), ('handed down', warm)):
        names = over.get((fixture, T, what), {})
        if not names:
            assert_certified(orc, X0, fix, rec, what=what)
            continue
        res, kind = residuals(orc, X0, fix, rec), classify(rec)
        assert not np.any(kind == 'skipped') and not np.any(kind == 'weak')
        exceeded = set()
        for cls, values in worst_per_class(res, kind).items():
            for name, value in values.items():
                if cls == 'polished' and name in names:
                    for i in np.flatnonzero((kind == cls) & ~(res[name] <= BASE[cls])):
                        exceeded.add(name)
                        assert res[name][i] <= min(names[name], _vertex_guarantee(orc, rec, i)[name]), (what, int(i), name, res[name][i])
                else:
                    assert value <= (0. if name.startswith('ray_') else BASE[cls]), (what, cls, name, value)
        assert exceeded == set(names), (what, exceeded)                    # (a bound nobody needs any more is to be taken out)


# ---------------------------------------------------------------------------------------------------------------------------
# planted defects
# ---------------------------------------------------------------------------------------------------------------------------
def _systems(which):
    if which == 'cart_pole_n20':
        orc = make_controller('cart_pole_with_walls', backend='oracle', threads=8)
        fix, _ = real_tree_with_parents(orc, X0)
        return orc, X0, fix
    if which == 'random_mld':                                              # (odd horizon, odd number of continuous inputs: n_dual = 379 is odd)
        return _random_mld_workload(5, 3, 2, 9, 21)
    return _config4_workload(64)


def _one(rec, i):
    return {k: v[i:i + 1].copy() for k, v in rec.items() if isinstance(v, np.ndarray)}


def _pick(ctrl, fix, rec):
    """A polished optimal record with what the defects need: fixed binaries with different positive nu_lb in two stages, an active
    mu row before the last stage and (where the last stage has rows of its own) an active row in the last stage."""
    cut, T, nub = ctrl.layout.dual_slices(), ctrl.T, ctrl.mld.nub
    for i in np.flatnonzero((rec['status'] == 0) & (rec['polished'] > 0)):
        d = rec['dual'][i]
        lb = np.array([d[cut['nu_lb'][t]] for t in range(T)])
        stages = [t for t in range(T) if np.any((lb[t] > 1e-6) & (fix[i].reshape(T, nub)[t] >= 0))]
        if len(stages) < 2 or not any(np.any(d[cut['mu'][t]] > 1e-6) for t in range(T - 1)):
            continue
        if ctrl.layout.ncL != ctrl.layout.nc and not np.any(d[cut['mu'][T - 1]] > 1e-6):
            continue
        return int(i)
    raise AssertionError('no record with the structure the planted defects need')


def _defect(ctrl, fix_row, row, name):
    """The dual row with one defect a kernel's write-out could have."""
    lay, T, nub = ctrl.layout, ctrl.T, ctrl.mld.nub
    cut, d = lay.dual_slices(), row.copy()
    fixed = fix_row.reshape(T, nub) >= 0
    if name == 'lam_one_stage_off':
        d[cut['lam'][0].start:cut['lam'][T].stop] = np.roll(row[cut['lam'][0].start:cut['lam'][T].stop], lay.nx)
    elif name == 'last_mu_block_with_the_stage_stride':
        o = cut['mu'][T - 1].start                                          # (written as if the last block were nc long: off by nc - ncL)
        d[o:o + lay.ncL] = np.roll(row[o:o + lay.ncL], lay.nc - lay.ncL)
    elif name == 'nu_lb_of_two_stages_swapped':
        cand = [(t, b) for t in range(T) for b in range(nub) if fixed[t, b] and row[cut['nu_lb'][t]][b] > 1e-6]
        (t0, b0) = cand[0]
        (t1, b1) = next((t, b) for t, b in cand if t != t0 and abs(row[cut['nu_lb'][t]][b] - row[cut['nu_lb'][t0]][b0]) > 1e-6)
        i0, i1 = cut['nu_lb'][t0].start + b0, cut['nu_lb'][t1].start + b1
        d[i0], d[i1] = row[i1], row[i0]
    elif name == 'nu_lb_and_nu_ub_exchanged':
        lo, hi = slice(cut['nu_lb'][0].start, cut['nu_lb'][T - 1].stop), slice(cut['nu_ub'][0].start, cut['nu_ub'][T - 1].stop)
        keep = ~fixed.ravel()                                               # (of the FIXED binaries: the free ones' pattern is what _dense_check reads)
        d[lo], d[hi] = np.where(keep, row[lo], row[hi]), np.where(keep, row[hi], row[lo])
    elif name == 'one_active_mu_scaled':
        t = next(t for t in range(T - 1) if np.any(row[cut['mu'][t]] > 1e-6))
        d[cut['mu'][t].start + int(np.argmax(row[cut['mu'][t]]))] *= 1. + 1e-5
    elif name == 'one_rho_zeroed':
        t = int(np.argmax([np.max(np.abs(row[cut['rho'][t]])) for t in range(T)]))
        d[cut['rho'][t]] = 0.
    elif name == 'sigma_of_the_binaries_dropped':
        for t in range(T):
            d[cut['sigma'][t]] = 0.
    elif name == 'fixed_binary_multiplier_not_split_by_sign':                # (nu_ub - nu_lb written to nu_ub whatever its sign: ONLY the signs see it)
        lo, hi = slice(cut['nu_lb'][0].start, cut['nu_lb'][T - 1].stop), slice(cut['nu_ub'][0].start, cut['nu_ub'][T - 1].stop)
        d[hi], d[lo] = np.where(fixed.ravel(), row[hi] - row[lo], row[hi]), np.where(fixed.ravel(), 0., row[lo])
    else:
        raise KeyError(name)
    assert not np.array_equal(d, row), name
    return d


OPTIMAL_DEFECTS = ('lam_one_stage_off', 'last_mu_block_with_the_stage_stride', 'nu_lb_of_two_stages_swapped', 'nu_lb_and_nu_ub_exchanged',
                   'one_active_mu_scaled', 'one_rho_zeroed', 'sigma_of_the_binaries_dropped')
# ... and three that exactly ONE residual sees (sign, dual_obj, gap): without them that residual could be taken out of assert_certified
SINGLE_RESIDUAL_DEFECTS = ('fixed_binary_multiplier_not_split_by_sign', 'dual_obj_of_the_last_iterate', 'dual_row_of_the_parent_node')
_CACHE = {}


def _solved(which):
    if which not in _CACHE:
        ctrl, x0, fix = _systems(which)
        _CACHE[which] = (ctrl, x0, fix, ctrl.qp.solve_batch(x0, fix))
    return _CACHE[which]


def _child_with_its_parents_row(ctrl, fix, rec):
    """(i, j): a polished optimal node i and its parent j whose record leaves the binary that i fixes without a multiplier: the
    parent's dual row and dual_obj in the child's slot -- the multipliers of ANOTHER node's batch slot -- are dual feasible for the
    child, consistent with their own dual_obj and a valid bound, but not the child's optimum."""
    cut = ctrl.layout.dual_slices()
    lb0, ub0 = cut['nu_lb'][0].start, cut['nu_ub'][0].start
    where = {f.tobytes(): j for j, f in enumerate(fix)}
    for i in np.flatnonzero((rec['status'] == 0) & (rec['polished'] > 0)):
        g, depth = fix[i].copy(), int((fix[i] >= 0).sum())
        if not depth:
            continue
        g[depth - 1] = -1
        j = where.get(g.tobytes(), -1)
        if j >= 0 and rec['status'][j] == 0 and rec['obj'][i] > rec['obj'][j] * (1 + 1e-4) \
                and rec['dual'][j][lb0 + depth - 1] == 0 and rec['dual'][j][ub0 + depth - 1] == 0:
            return int(i), int(j)
    raise AssertionError('no child whose parent leaves the branched binary without a multiplier')


SYSTEMS = ('cart_pole_n20', 'random_mld', 'config4')
# what does not exist for a system is not in the list: without a terminal set the last stage has the rows of every stage (nc == ncL),
# and only the real tree of the cart-pole holds parents beside their children
PLANTED = [(w, d) for w in SYSTEMS for d in OPTIMAL_DEFECTS + SINGLE_RESIDUAL_DEFECTS + ('ray_with_a_nonzero_rho', 'ray_scaled_by_minus_one')
           if w == 'cart_pole_n20' or d not in ('last_mu_block_with_the_stage_stride', 'dual_row_of_the_parent_node')]


@pytest.mark.parametrize('which,defect', PLANTED)
def test_planted_defects_are_caught(which, defect):
    ctrl, x0, fix, rec = _solved(which)
    lay = ctrl.layout
    assert which != 'random_mld' or lay.n_dual % 2 == 1
    assert defect != 'last_mu_block_with_the_stage_stride' or lay.nc != lay.ncL
    if defect.startswith('ray'):
        i = int(np.flatnonzero((rec['status'] == 1) & (rec['weak'] == 0))[0])
        one = _one(rec, i)
        assert_certified(ctrl, x0, fix[i:i + 1], one)
        if defect == 'ray_with_a_nonzero_rho':
            one['dual'][0, lay.dual_slices()['rho'][1].start] = 1e-12
        else:
            one['dual'] *= -1.
            one['dual_obj'] *= -1.
        with pytest.raises(AssertionError, match='fails its certificate'):
            assert_certified(ctrl, x0, fix[i:i + 1], one)
        return
    i = _pick(ctrl, fix, rec)
    if defect == 'dual_row_of_the_parent_node':
        i, j = _child_with_its_parents_row(ctrl, fix, rec)
    clean, bad = _one(rec, i), _one(rec, i)
    assert_certified(ctrl, x0, fix[i:i + 1], clean)
    if defect == 'dual_obj_of_the_last_iterate':                            # (the scalar, not the row: a value from before the polish)
        bad['dual_obj'] *= 1. + 1e-6
    elif defect == 'dual_row_of_the_parent_node':
        bad['dual'][0], bad['dual_obj'][0] = rec['dual'][j], rec['dual_obj'][j]
    else:
        bad['dual'][0] = _defect(ctrl, fix[i], rec['dual'][i], defect)
    with pytest.raises(AssertionError, match='fails its certificate'):
        assert_certified(ctrl, x0, fix[i:i + 1], bad, ref=clean)
    if defect in SINGLE_RESIDUAL_DEFECTS:
        return
    # ... and the comparison with the oracle that the GPU tests made of an optimal record until now does NOT notice: status, obj,
    # dual_obj (the solver's own scalar) and trajectories are untouched, the signs _dense_check reads the active set from as well
    from test_gpu_parity import _compare, _dense_check
    if defect != 'last_mu_block_with_the_stage_stride':                    # (that one moves active rows: the dense solve does see another set)
        _dense_check(ctrl, ctrl.T, x0, fix[i:i + 1], bad)
    _compare(ctrl, bad, clean, ctrl.T, fix[i:i + 1])


def _raised(ctrl, x0, fix_rows, bad):
    """The residuals of a one-record batch that lie over what assert_certified holds it to without a reference."""
    import certificates
    res, cls = residuals(ctrl, x0, fix_rows, bad), classify(bad)[0]
    return [k for k in certificates._names(cls) if not res[k][0] <= (0. if k in certificates.EXACT else BASE[cls])]


def _single_fault(name):
    """One-record batches (fix rows, record) on the cart-pole's real tree whose ONLY fault is the residual ``name``."""
    ctrl, x0, fix, rec = _solved('cart_pole_n20')
    i = _pick(ctrl, fix, rec)
    bad, rows = _one(rec, i), fix[i:i + 1]
    ray = int(np.flatnonzero((rec['status'] == 1) & (rec['weak'] == 0))[0])
    if name == 'stationarity':
        bad['dual'][0] = _defect(ctrl, fix[i], rec['dual'][i], 'nu_lb_of_two_stages_swapped')
    elif name == 'sign':
        bad['dual'][0] = _defect(ctrl, fix[i], rec['dual'][i], 'fixed_binary_multiplier_not_split_by_sign')
    elif name == 'dual_obj':
        bad['dual_obj'] *= 1. + 1e-6
    elif name == 'gap':
        i, j = _child_with_its_parents_row(ctrl, fix, rec)
        bad, rows = _one(rec, i), fix[i:i + 1]
        bad['dual'][0], bad['dual_obj'][0] = rec['dual'][j], rec['dual_obj'][j]
    elif name == 'obj':                                                      # (the scalar of another iterate beside the vertex)
        bad['obj'] *= 1. + 1e-6
    elif name in ('primal_equality', 'primal_inequality'):
        # one entry of the primal row off by 1e-6 (a neighbour's value, a stale store): which entries show in the dynamics alone and
        # which in a bound alone depends on the system -- the first entry whose only trace is the residual asked for
        for k in range(ctrl.layout.n_primal):
            for step in (1e-6, -1e-6):
                bad = _one(rec, i)
                bad['primal'][0, k] += step
                if _raised(ctrl, x0, rows, bad) == [name]:
                    return [(rows, bad)]
        raise AssertionError('no entry of the primal row shows in %s alone' % name)
    elif name == 'ray_quadratic':
        bad = _one(rec, ray)
        bad['dual'][0, ctrl.layout.dual_slices()['rho'][1].start] = 1e-12
        rows = fix[ray:ray + 1]
    elif name == 'ray_objective':
        # the ray of ANOTHER node's slot, with the dual_obj that goes with it at this node: stationary, signs right, consistent -- and no
        # proof: the node is feasible, so no ray has a positive dual objective there
        from kkt_checks import dual_objective
        from certificates import identifier_of
        from warm_start_hmpc_amd.subproblem_solution import DualSolution
        bad = _one(rec, ray)
        variables = DualSolution.from_row(ctrl.layout, 0., rec['dual'][ray]).variables
        bad['dual_obj'][0] = dual_objective(ctrl, variables, identifier_of(fix[i], ctrl.mld.nub), x0)
        assert bad['dual_obj'][0] <= 0.
    elif name == 'ray_primal':
        first, second = _one(rec, ray), _one(rec, ray)
        first['primal'][0, 3] = 0.                                           # one entry of the primal row written, ...
        second['obj'][0] = 1.                                                # ... a finite objective beside a ray
        return [(fix[ray:ray + 1], first), (fix[ray:ray + 1], second)]
    else:
        raise KeyError(name)
    return [(rows, bad)]


@pytest.mark.parametrize('name', sorted(set(OPTIMAL + RAY)))
def test_removing_a_residual_lets_a_planted_defect_through(monkeypatch, name):
    # every residual assert_certified holds is the ONLY one that catches some planted defect: assert_certified refuses the record
    # naming that residual, and accepts it once the residual is taken out of the list of the record's class
    import certificates
    ctrl, x0, _, _ = _solved('cart_pole_n20')
    cases = _single_fault(name)
    for rows, bad in cases:
        assert _raised(ctrl, x0, rows, bad) == [name]
        with pytest.raises(AssertionError, match='fails its certificate: %s = ' % name):
            assert_certified(ctrl, x0, rows, bad)
    inner = certificates._names
    monkeypatch.setattr(certificates, '_names', lambda cls: tuple(k for k in inner(cls) if k != name))
    for rows, bad in cases:
        assert_certified(ctrl, x0, rows, bad)


def test_records_land_in_their_class():
    orc = make_controller('cart_pole_with_walls', T=10, backend='oracle', threads=8)
    x0 = np.array([0., 0., .5, 0.])
    fix = random_prefix_frontier(10, 4, 64, p_one=0.1)
    fix[0, :] = -1
    rec = orc.qp.solve_batch(x0, fix)
    base = assert_certified(orc, x0, fix, rec)
    opt, inf = np.flatnonzero(rec['status'] == 0), np.flatnonzero(rec['status'] == 1)
    # an undecided node (status > 1) is counted, not dropped -- whatever its rows hold
    r = {k: v.copy() for k, v in rec.items() if isinstance(v, np.ndarray)}
    r['status'][opt[0]] = 2
    r['dual'][opt[0]] = np.nan
    counts = assert_certified(orc, x0, fix, r)
    assert counts['skipped'] == 1 and counts['polished'] == base['polished'] - 1
    # an unpolished record is held to its own base: a KKT point to 1e-7 passes there and fails as a polished one
    r = {k: v.copy() for k, v in rec.items() if isinstance(v, np.ndarray)}
    cut = orc.layout.dual_slices()
    r['dual'][opt[1], cut['lam'][3].start] += 1e-7 * (1 + np.abs(r['dual'][opt[1]]).max())
    with pytest.raises(AssertionError, match='polished record %d fails its certificate: stationarity' % opt[1]):
        assert_certified(orc, x0, fix, r)
    r['polished'][opt[1]] = 0
    counts = assert_certified(orc, x0, fix, r)
    assert counts['unpolished'] == 1 and counts['polished'] == base['polished'] - 1
    # a handed-down record (the oracle marks it attempt 64) is a polished one
    handed = orc.qp.solve_batch(x0, fix[opt[:4]], warm=(rec['primal'], rec['dual'], opt[:4].astype(np.int32)))
    assert np.all(handed['polished'] == 64) and assert_certified(orc, x0, fix[opt[:4]], handed)['polished'] == 4
    # a WEAK ray is exempt from the stationarity bound ONLY, and only one per hundred infeasible records may be WEAK
    r = {k: v.copy() for k, v in rec.items() if isinstance(v, np.ndarray)}
    r['dual'][inf[0], cut['lam'][2].start] += 1e-3
    with pytest.raises(AssertionError, match='infeasible record %d fails its certificate: stationarity' % inf[0]):
        assert_certified(orc, x0, fix, r)
    r['weak'][inf[0]] = 1
    assert assert_certified(orc, x0, fix, r)['weak'] == 1
    r['dual'][inf[0], cut['rho'][0].start] = 1e-9
    with pytest.raises(AssertionError, match='weak record %d fails its certificate: ray_quadratic' % inf[0]):
        assert_certified(orc, x0, fix, r)
    r['dual'][inf[0], cut['rho'][0].start] = 0.
    r['weak'][inf[1]] = 1
    with pytest.raises(AssertionError, match='WEAK rays'):
        assert_certified(orc, x0, fix, r)
    # the reference widens a bound only where ITS OWN residual of that class is large
    r = {k: v.copy() for k, v in rec.items() if isinstance(v, np.ndarray)}
    r['dual'][opt[1], cut['lam'][3].start] += 1e-7 * (1 + np.abs(r['dual'][opt[1]]).max())
    with pytest.raises(AssertionError, match='stationarity'):
        assert_certified(orc, x0, fix, r, ref=rec)
    assert_certified(orc, x0, fix, rec, ref=r)                              # (4 x 1e-7 admits the clean records, and nothing else changes)
