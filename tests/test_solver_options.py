"""The QP solvers held to every option of ``hmpc_options`` (include/hmpc.h): tol, tol_inf, max_iter, lazy_terminal, refine, polish,
polish_tol.  The checks are the plain functions of tests/option_checks.py.  Without a GPU: the oracle passes all of them on every
case of the matrix and every problem (which makes the bounds of the GPU part a comparison with the reference, not with the code
under test), and planted defects fail the check that is there for them, by name.  Marked gpu: the kernels -- the default one of
each problem, the shipped instantiations, the run-time-sized kernel and its streaming form -- on the same matrix.

Every number in here is exact (bitwise, counts, caps), an option's own value, or a ratio measured on the ORACLE with its margin
(option_checks.option_is_felt).  What the kernels measure goes to DESIGN.md 3.14, not into a bound."""
import contextlib
import os

import numpy as np
import pytest

from helpers import make_controller, random_prefix_frontier, random_mld, real_tree_with_parents, dive_and_prefix_frontier, _NoBackend
from certificates import new_margins, residuals
from option_checks import (DEFAULTS, TIGHT, effective, passes_of, handed, same_records, decisions_agree, bracketed, bracket_delta, _parts,
                           certified_at, truncated, capped_iters, option_is_felt, all_checks, worst_of, options_line, bases_at)
from oracle.oracle_qp import OracleBatchedQP

CASES = {
    'polish0': dict(polish=0), 'refine0': dict(refine=0), 'lazy0': dict(lazy_terminal=0),
    'polish0_refine0': dict(polish=0, refine=0), 'polish0_lazy0': dict(polish=0, lazy_terminal=0),
    'tol1e-6_polish0': dict(tol=1e-6, polish=0), 'tol1e-10_polish0': dict(tol=1e-10, polish=0),
    'tol1e-5_ptol1e-3': dict(tol=1e-5, polish_tol=1e-3), 'ptol1e-7': dict(polish_tol=1e-7), 'ptol1e-2': dict(polish_tol=1e-2),
    'tolinf1e-4': dict(tol_inf=1e-4), 'tolinf1e-9': dict(tol_inf=1e-9),
    'cap8': dict(max_iter=8), 'cap12': dict(max_iter=12), 'cap12_lazy0': dict(max_iter=12, lazy_terminal=0),
    'cap10_polish0_lazy0': dict(max_iter=10, polish=0, lazy_terminal=0),
    'cap3': dict(max_iter=3),                                        # (everything undecided)
}
CONTROL_FLOW = ('polish0_lazy0', 'lazy0', 'refine0', 'cap12_lazy0', 'cap8')     # the cases that change the kernels' control flow

# name: (fixture, T, x0, terminal set, nodes of the tree that are kept) or (nx, nuc, nub, seed, T) of helpers.random_mld; and the
# split optimal / infeasible of the oracle at the defaults
PROBLEMS = {
    'walls10': (('cart_pole_with_walls', 10, (0., 0., .5, 0.), True, None), (43, 101)),
    'walls20': (('cart_pole_with_walls', 20, (0., 0., 1., 0.), True, None), (82, 142)),
    'walls40': (('cart_pole_with_walls', 40, (0., 0., 1., 0.), True, 192), (97, 159)),
    'one_wall20': (('cart_pole_one_wall', 20, (0., 0., 1., 0.), True, None), (46, 95)),
    'mld8': ((8, 3, 4, 2, 10), (83, 77)),
    'mld10': ((10, 4, 4, 5, 8), (83, 77)),
    'walls20_no_terminal': (('cart_pole_with_walls', 20, (0., 0., 1., 0.), False, None), None),     # (truncated only)
}
SIX = ('walls10', 'walls20', 'walls40', 'one_wall20', 'mld8', 'mld10')
_WORK, _ORACLE = {}, {}


def _workload(name):
    """(controller, x0, fix, parent): the real tree of a cold search plus 64 random prefixes (cart-poles), the dives and prefixes of
    helpers.dive_and_prefix_frontier (random MLDs).  parent: index of each node's parent in the batch, or -1."""
    if name not in _WORK:
        spec = PROBLEMS[name][0]
        if isinstance(spec[0], str):
            fixture, T, x0, terminal, keep = spec
            x0 = np.array(x0)
            ctrl = make_controller(fixture, T=T, terminal=terminal, backend='oracle', threads=8)
            fix, parent = real_tree_with_parents(ctrl, x0)
            if keep:
                fix, parent = fix[:keep], np.where(parent[:keep] < keep, parent[:keep], -1).astype(np.int32)
            fix = np.concatenate((fix, random_prefix_frontier(T, ctrl.mld.nub, 64, seed0=1000)))
            parent = np.concatenate((parent, np.full(64, -1, np.int32)))
        else:
            from warm_start_hmpc_amd.controller import HybridModelPredictiveController
            nx, nuc, nub, seed, T = spec
            mld, objective, x0 = random_mld(nx=nx, nuc=nuc, nub=nub, seed=seed)
            ctrl = HybridModelPredictiveController(mld, T, objective, None, backend=_NoBackend())
            ctrl.qp = OracleBatchedQP(ctrl.problem_data(), threads=8)
            fix = dive_and_prefix_frontier(ctrl.qp, mld, x0, T, seed)
            parent = np.full(len(fix), -1, np.int32)
        _WORK[name] = (ctrl, x0, fix, parent)
    return _WORK[name]


def _oracle(name, warm=None, **options):
    """The oracle's records of a workload at these options (computed once, shared, never written to)."""
    key = (name, tuple(sorted(options.items())))
    if warm is not None or key not in _ORACLE:
        ctrl, x0, fix, _ = _workload(name)
        rec = OracleBatchedQP(ctrl.problem_data(), threads=8, **options).solve_batch(x0, fix, warm=warm)
        if warm is not None:
            return rec
        _ORACLE[key] = rec
    return _ORACLE[key]


def _copy(rec):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in rec.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('name', SIX)
def test_the_oracle_passes_every_check_on_every_case(name, case):
    ctrl, x0, fix, _ = _workload(name)
    default, tight, rec = _oracle(name), _oracle(name, **TIGHT), _oracle(name, **CASES[case])
    assert ((default['status'] == 0).sum(), (default['status'] == 1).sum()) == PROBLEMS[name][1] and len(fix) == sum(PROBLEMS[name][1])
    assert np.all(tight['status'] <= 1) and np.array_equal(tight['status'], default['status'])
    # The oracle beside ITSELF would pass any bound that its own residual widens: it is held to the bases alone -- but for the polished
    # class, which may lie at 4 x the oracle's records at the DEFAULT options (pinned by test_certificates.py: a vertex verified on unit
    # rows misses 1e-8 on a row of large norm, and does so whatever the options)
    used = all_checks(ctrl, x0, fix, rec, default, tight, CASES[case], what='%s %s' % (name, case), widen=('polished',))
    assert used <= 1.
    if case == 'cap3':
        assert np.all(rec['status'] == 2)
    if 'max_iter' not in CASES[case]:
        assert np.array_equal(rec['status'], default['status'])


SINGLE_PASS = (('walls10', dict(lazy_terminal=0)), ('walls20', dict(lazy_terminal=0)), ('walls20_no_terminal', {}), ('one_wall20', dict(lazy_terminal=0)))


@pytest.mark.parametrize('polish', [1, 0])
@pytest.mark.parametrize('name,options', SINGLE_PASS)
def test_a_capped_solve_of_the_oracle_is_the_uncapped_one_cut_off(name, options, polish):
    ctrl = _workload(name)[0]
    assert passes_of(ctrl, options) == 1
    u = _oracle(name, polish=polish, **options)
    for cap in (8, 10, 12):
        counts = truncated(u, _oracle(name, polish=polish, max_iter=cap, **options), cap, what=name)
        assert min(counts) >= 1, (name, cap, counts)
    if name == 'walls10':                                             # (the partition is not a trivial one)
        assert min(truncated(u, _oracle(name, polish=polish, max_iter=10, **options), 10)) >= 3


def test_the_iteration_cap_is_one_per_pass():
    # with the terminal set tried lazily a node may be solved twice: the count is the sum of both passes (2 x cap is reached at the
    # small caps), and in one pass the cap itself is reached
    for cap in (3, 8, 12):
        lazy, single = _oracle('walls10', max_iter=cap), _oracle('walls10', max_iter=cap, lazy_terminal=0)
        assert cap < capped_iters(lazy, cap, 2) <= 2 * cap and capped_iters(single, cap, 1) == cap
        assert cap == 12 or capped_iters(lazy, cap, 2) == 2 * cap
        with pytest.raises(AssertionError, match='^capped_iters: '):
            capped_iters(lazy, cap, 1)


class _Dropping(object):
    """A backend that never hands one option on: the solver runs with the default of it."""

    def __init__(self, name, dropped):
        self.name, self.dropped = name, dropped

    def __call__(self, **options):
        return _oracle(self.name, **{k: v for k, v in options.items() if k != self.dropped})


@pytest.mark.parametrize('dropped', ['max_iter', 'tol_inf', 'polish', 'polish_tol'])
def test_a_backend_that_drops_an_option_is_caught(dropped):
    ctrl, x0, fix, _ = _workload('walls10')
    solve = _Dropping('walls10', dropped)
    if dropped == 'max_iter':
        capped_iters(_oracle('walls10', max_iter=8), 8, 2)
        with pytest.raises(AssertionError, match='^capped_iters: .* ran \\d+ iterations'):
            capped_iters(solve(max_iter=8), 8, 2)
        return
    option_is_felt(ctrl, lambda **o: _oracle('walls10', **o))
    with pytest.raises(AssertionError, match='^option_is_felt: .*%s' % {'tol_inf': 'tol_inf does not reach the rays', 'polish': 'polish = 0 returns',
                                                                        'polish_tol': 'polish_tol does not move'}[dropped]):
        option_is_felt(ctrl, solve)


@pytest.mark.parametrize('name', ['walls10', 'walls20', 'one_wall20'])
def test_the_ratios_of_the_oracle_leave_their_margins(name):
    got = option_is_felt(_workload(name)[0], lambda **o: _oracle(name, **o), what=name)
    assert got['tol_inf_ratio'] <= 1e-4                              # (two decades below what option_is_felt asks)


def test_planted_defects_in_records_are_caught():
    ctrl, x0, fix, _ = _workload('walls10')
    tight = _oracle('walls10', **TIGHT)
    # one extra iteration in the iteration word
    options = dict(max_iter=12, lazy_terminal=0)
    rec = _copy(_oracle('walls10', **options))
    capped_iters(rec, 12, 1)
    rec['iters'][int(np.argmax(rec['iters']))] += 1
    with pytest.raises(AssertionError, match='^capped_iters: .* ran 13 iterations'):
        capped_iters(rec, 12, 1)
    # an undecided record that carries a flag of a decided one
    rec = _copy(_oracle('walls10', **options))
    und = int(np.flatnonzero(rec['status'] == 2)[0])
    rec['polished'][und] = 1
    with pytest.raises(AssertionError, match='^capped_iters: .*undecided record %d .* carries POLISHED' % und):
        capped_iters(rec, 12, 1)
    # a capped run with one record "below" the cap off in the last bit of one dual entry
    u, r = _oracle('walls10', lazy_terminal=0), _copy(_oracle('walls10', **options))
    truncated(u, r, 12)
    i = int(np.flatnonzero((u['iters'] < 12) & (u['status'] == 0))[0])
    k = int(np.argmax(np.abs(r['dual'][i])))
    r['dual'][i, k] = np.nextafter(r['dual'][i, k], np.inf)
    with pytest.raises(AssertionError, match='^truncated: .*dual differs in 1 records, first %d' % i):
        truncated(u, r, 12)
    # ... a node over the cap that is decided after all, and one that turns INFEASIBLE under the cap
    r = _copy(_oracle('walls10', **options))
    j = int(np.flatnonzero(u['iters'] > 12)[0])
    r['status'][j], r['iters'][j] = 0, 11                              # (OPTIMAL after exactly 12 would be the acceptable iterate the cap falls on)
    with pytest.raises(AssertionError, match='^truncated: .*node %d took' % j):
        truncated(u, r, 12)
    r['status'][j] = 1
    with pytest.raises(AssertionError, match='^truncated: '):
        truncated(u, r, 12)
    # an OPTIMAL record whose obj lies 10 delta lower
    rec = _copy(_oracle('walls10', polish=0))
    i = int(np.flatnonzero(rec['status'] == 0)[3])
    below, above = bracket_delta(_parts(ctrl, x0, fix[i], rec, i), _parts(ctrl, x0, fix[i], tight, i))
    t = _parts(ctrl, x0, fix[i], tight, i)
    delta = above + abs(t['p'] - t['d']) + sum(bracket_delta(t, t)) + 4 * (len(rec['primal'][i]) + len(rec['dual'][i])) * 2. ** -52 * (1 + abs(t['p']))
    assert bracketed(ctrl, x0, fix, rec, tight) <= 1. and delta < 1e-6 * (1 + rec['obj'][i])
    rec['obj'][i] -= 10 * delta
    with pytest.raises(AssertionError, match='^bracketed: .*record %d does not bracket the tight optimum \\(reported\\)' % i):
        bracketed(ctrl, x0, fix, rec, tight)
    # ... and a decision that moves
    rec = _copy(_oracle('walls10'))
    rec['status'][i] = 1
    with pytest.raises(AssertionError, match='^decisions_agree: 1 decided nodes contradict'):
        decisions_agree(rec, tight)
    rec['status'][i] = 2
    decisions_agree(rec, tight, capped=True)
    with pytest.raises(AssertionError, match='^decisions_agree: 1 nodes undecided without a cap'):
        decisions_agree(rec, tight)


def test_the_class_bases_follow_the_options():
    ctrl, x0, fix, _ = _workload('walls20')
    assert bases_at(ctrl, {}) == {'polished': 1e-8, 'unpolished': 5e-6, 'infeasible': 1e-6, 'weak': 1e-6}      # certificates.BASE
    assert bases_at(ctrl, dict(tol=1e-10, tol_inf=1e-9))['unpolished'] == 5e-6 and bases_at(ctrl, dict(tol_inf=1e-9))['infeasible'] == 1e-9
    assert bases_at(ctrl, dict(tol=1e-6))['unpolished'] == 5e-4 and bases_at(ctrl, dict(tol=1e-5, polish_tol=1e-3))['polished'] == 1e-8
    # a ray that is a proof to 1e-6 is none at tol_inf = 1e-9
    rec = _oracle('walls20')
    certified_at(ctrl, x0, fix, rec, None, {})
    with pytest.raises(AssertionError, match='^certified_at: .*infeasible record \\d+ fails its certificate: stationarity'):
        certified_at(ctrl, x0, fix, rec, None, dict(tol_inf=1e-9))
    # refine = 0: the unpolished records that left at the floor of the barrier parameter miss the base of 5e-6 by
    # their gap alone and meet the stated contract, 100 tol x the largest entry of the cost's Hessian; the reference does not widen it
    options = dict(polish=0, refine=0)
    rec = _oracle('walls20', **options)
    res = residuals(ctrl, x0, fix, rec)
    late = np.flatnonzero(res['gap'] > 5e-6)
    assert late.size >= 3 and np.all(rec['status'][late] == 0) and np.nanmax(res['stationarity'][rec['status'] == 0]) <= 5e-6
    bound = bases_at(ctrl, options)['unpolished']
    assert bound[None] == 5e-6 and 3e-5 < bound['gap'] == 1e-6 * 2. * max((ctrl.Q.T.dot(ctrl.Q)).max(), (ctrl.Q_T.T.dot(ctrl.Q_T)).max(), (ctrl.R.T.dot(ctrl.R)).max()) < 4e-5
    certified_at(ctrl, x0, fix, rec, rec, options)
    with pytest.raises(AssertionError, match='^certified_at: .*unpolished record \\d+ fails its certificate: gap'):
        certified_at(ctrl, x0, fix, rec, None, dict(polish=0))
    worse = _copy(rec)
    worse['dual'][late[0]] *= 1. + 1e-3                               # (gap 1e-3: over the contract, and 4 x the reference's own gap is no excuse)
    worse['dual_obj'][late[0]] *= 1. + 1e-3
    with pytest.raises(AssertionError, match='^certified_at: .*unpolished record %d fails its certificate' % late[0]):
        certified_at(ctrl, x0, fix, worse, rec, options)


ZEROS = dict(tol=0., tol_inf=-1., max_iter=0, polish_tol=-1e-4)      # (the switches stay as they are: 0 means off)


def test_the_restated_mapping_of_zero_and_negative_fields_mirrors_hmpc_create():
    # The oracle maps nothing itself: what is held here is option_checks.effective(), the restatement of build_host_problem's mapping
    # that every check above runs on (the last line only shows that the mapped options ARE the default solve).  The mapping of the
    # library itself is held through the C ABI, in test_zero_and_negative_option_fields_through_the_c_abi.
    assert effective(dict(ZEROS, lazy_terminal=1, refine=1, polish=1)) == DEFAULTS
    assert effective(dict(tol=0., polish=0)) == dict(DEFAULTS, polish=0) and effective(dict(max_iter=-5, lazy_terminal=0)) == dict(DEFAULTS, lazy_terminal=0)
    with pytest.raises(KeyError):
        effective(dict(device=0))
    same_records(_oracle('walls10', **effective(ZEROS)), _oracle('walls10'))


def test_the_oracle_hands_nothing_down_without_the_polish():
    ctrl, x0, fix, parent = _workload('walls10')
    cold = _oracle('walls10', polish=0)
    index = np.where((parent >= 0) & (cold['status'][np.maximum(parent, 0)] == 0), parent, -1).astype(np.int32)
    assert (index >= 0).sum() >= 20
    warm = _oracle('walls10', warm=(cold['primal'], cold['dual'], index), polish=0)
    same_records(warm, cold, what='handed down without the polish')
    assert not handed(warm).any()


# ---------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(**values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update({k: str(v) for k, v in values.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


FAMILIES = {                                                         # environment that selects a kernel family, and the kinds hmpc_kernel_info names
    'default': ({}, None),
    'shipped_w1': (dict(HMPC_JIT_SIZED=0, HMPC_WAVES=1), (2, 2, 2)), 'shipped_w2': (dict(HMPC_JIT_SIZED=0, HMPC_WAVES=2), (2, 2, 2)),
    'shipped_w4': (dict(HMPC_JIT_SIZED=0, HMPC_WAVES=4), (2, 2, 2)),
    'generic': (dict(HMPC_FORCE_GENERIC=1), (0, 0, 0)),
    'streaming': (dict(HMPC_FORCE_BIG=1), (1, 1, 1)),
}
TABLE = {}


def _hip(name, family='default', warm=None, selfcheck=True, **options):
    """The kernel's records of a workload: a handle of its own per call (the options are the handle's), the family's environment
    around creation and solve."""
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    ctrl, x0, fix, _ = _workload(name)
    env, kinds = FAMILIES[family]
    with _env(**dict(env, **({} if selfcheck else dict(HMPC_JIT_SELFCHECK=0)))):
        qp = HipBatchedQP(ctrl.problem_data(), **options)
        # (the default kernels are compiled with the problem's sizes: kinds 4 / 5 / 6 of hmpc_kernel_info)
        assert qp.kernel_info() == kinds if kinds else min(qp.kernel_info()) >= 4, (name, family, qp.kernel_info())
        return qp.solve_batch(x0, fix, warm=warm)


@pytest.fixture(scope='module')
def report():
    yield
    if TABLE:
        print('\n' + options_line(TABLE))


def _hold(name, case, family='default', table=False):
    ctrl, x0, fix, _ = _workload(name)
    margins = new_margins()
    rec = _hip(name, family, **CASES[case])
    used = all_checks(ctrl, x0, fix, rec, _oracle(name, **CASES[case]), _oracle(name, **TIGHT), CASES[case], what='%s %s %s' % (name, family, case), margins=margins)
    assert used <= 1.
    if table:
        TABLE[case] = worst_of(margins) + (used,)
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(CASES))
def test_default_kernel_on_every_case(report, case):
    rec = _hold('walls10', case, table=True)
    if case == 'cap3':
        assert np.all(rec['status'] == 2)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CONTROL_FLOW)
@pytest.mark.parametrize('name', ['walls20', 'one_wall20', 'mld8', 'mld10'])
def test_default_kernels_of_other_problems_on_the_cases_that_change_control_flow(name, case):
    _hold(name, case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CONTROL_FLOW)
@pytest.mark.parametrize('family', [f for f in FAMILIES if f != 'default'])
def test_other_kernel_families_on_the_cases_that_change_control_flow(family, case):
    _hold('walls10', case, family)


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['default', 'shipped_w1', 'shipped_w2', 'shipped_w4', 'streaming'])
@pytest.mark.parametrize('name,options', [('walls10', dict(lazy_terminal=0, polish=1)), ('walls10', dict(lazy_terminal=0, polish=0)), ('walls20_no_terminal', {})])
def test_a_capped_solve_of_one_binary_is_its_uncapped_one_cut_off(name, options, family):
    # one binary against ITSELF (no second opinion of another kernel: HMPC_JIT_SELFCHECK=0); the partition comes from the kernel's
    # own uncapped iteration counts, and is no trivial one
    u = _hip(name, family, selfcheck=False, **options)
    below, at, above = truncated(u, _hip(name, family, selfcheck=False, max_iter=10, **options), 10, what='%s %s' % (name, family))
    assert min(below, at, above) >= 3, (below, at, above)
    print('%s %s %s: below / at / above the cap of 10: %d / %d / %d' % (name, family, options, below, at, above))
    for cap in (8, 12):
        truncated(u, _hip(name, family, selfcheck=False, max_iter=cap, **options), cap, what='%s %s' % (name, family))


def _device_records(qp, x0, fix, warm=None):
    import torch
    dev, B = torch.device('cuda', 0), len(fix)
    out = dict(obj=torch.empty(B, dtype=torch.float64, device=dev), dual_obj=torch.empty(B, dtype=torch.float64, device=dev),
               status=torch.empty(B, dtype=torch.int32, device=dev), iters=torch.empty(B, dtype=torch.int32, device=dev),
               primal=torch.empty(B, qp.n_primal, dtype=torch.float64, device=dev), dual=torch.empty(B, qp.n_dual, dtype=torch.float64, device=dev))
    qp.solve_batch_device(torch.from_numpy(x0).to(dev), torch.from_numpy(fix).to(dev), out, warm=warm)
    torch.cuda.synchronize()
    rec = {k: v.cpu().numpy() for k, v in out.items()}
    word = rec['iters']
    rec.update(handed=(word >> 18) & 1, polished=(word >> 16) & 1, weak=(word >> 17) & 1, uncertified=(word >> 20) & 1, second=(word >> 19) & 1, iters=word & 0xFFFF)
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize('entry', ['host', 'device'])
def test_the_second_opinion_under_an_iteration_cap(entry):
    # cap8 leaves most nodes undecided: the shipped kernel is asked for all of them, with the same options -- decisions and certificates
    # hold, the runs are counted, and the first-use check (in the same call) does not take the cap for a defect of the compiled kernel
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    ctrl, x0, fix, _ = _workload('walls10')
    qp = HipBatchedQP(ctrl.problem_data(), **CASES['cap8'])
    kinds = qp.kernel_info()
    assert min(kinds) >= 4
    rec = qp.solve_batch(x0, fix) if entry == 'host' else _device_records(qp, x0, fix)
    assert (rec['status'] == 2).sum() >= 20
    assert qp.kernel_info() == kinds                                  # (not dropped by the first-use check)
    ref, tight = _oracle('walls10', **CASES['cap8']), _oracle('walls10', **TIGHT)
    decisions_agree(rec, tight, capped=True)
    capped_iters(rec, 8, 2)
    certified_at(ctrl, x0, fix, rec, ref, CASES['cap8'])
    dropped, second_runs, _ = qp.jit_stats()                           # (takes in the counts of the second opinion: the review)
    assert second_runs >= 1 and dropped == 0 and qp.kernel_info() == kinds      # (nor dropped by the review: the shipped kernel is capped alike)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['polish0_lazy0', 'cap12'])
def test_the_device_entry_returns_the_host_entrys_records(case):
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    ctrl, x0, fix, _ = _workload('walls10')
    qp = HipBatchedQP(ctrl.problem_data(), **CASES[case])
    same_records(_device_records(qp, x0, fix), qp.solve_batch(x0, fix), what='device entry, %s' % case)


@pytest.mark.gpu
def test_hand_down_under_options():
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    ctrl, x0, fix, parent = _workload('walls10')
    # without the polish nothing is handed down: the cold records, bit for bit
    qp = HipBatchedQP(ctrl.problem_data(), polish=0)
    cold = qp.solve_batch(x0, fix)
    index = np.where((parent >= 0) & (cold['status'][np.maximum(parent, 0)] == 0), parent, -1).astype(np.int32)
    assert (index >= 0).sum() >= 20
    warm = qp.solve_batch(x0, fix, warm=(cold['primal'], cold['dual'], index))
    same_records(dict(warm, second=None), cold, what='handed down without the polish')   # (HMPC_ITERS_TERMINAL is raised by launches with hmpc_warm only)
    assert not warm['handed'].any() and not warm['polished'].any()
    # every terminal-set row live from the first iteration, polish on: verified hand-downs certify, decisions are the cold ones
    options = dict(lazy_terminal=0)
    qp = HipBatchedQP(ctrl.problem_data(), **options)
    cold = qp.solve_batch(x0, fix)
    index = np.where((parent >= 0) & (cold['status'][np.maximum(parent, 0)] == 0) & (cold['polished'][np.maximum(parent, 0)] > 0), parent, -1).astype(np.int32)
    warm = qp.solve_batch(x0, fix, warm=(cold['primal'], cold['dual'], index))
    orc = _oracle('walls10', **options)
    owarm = _oracle('walls10', warm=(orc['primal'], orc['dual'], index), **options)
    assert warm['handed'].sum() >= 10 and handed(owarm).sum() >= 10
    assert np.array_equal(warm['status'], cold['status'])
    certified_at(ctrl, x0, fix, warm, owarm, options, what='handed down, lazy_terminal = 0')
    assert bracketed(ctrl, x0, fix, warm, _oracle('walls10', **TIGHT)) <= 1.


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['walls10', 'one_wall20'])
def test_every_option_is_felt_by_the_kernel(name):
    got = option_is_felt(_workload(name)[0], lambda **o: _hip(name, **o), what=name)
    print('%s: %r' % (name, got))


@pytest.mark.gpu
def test_zero_and_negative_option_fields_through_the_c_abi():
    # hmpc_create with the struct as a C caller would zero it (and with negative values): the records of the defaults, bit for bit
    from warm_start_hmpc_amd import qp_backend
    ctrl, x0, fix, _ = _workload('walls10')
    default = qp_backend.HipBatchedQP(ctrl.problem_data()).solve_batch(x0, fix)
    seen = []
    real = qp_backend._Options

    def raw(**kw):                                                       # the struct HipBatchedQP fills, with the fields under test replaced
        o = real(**kw)
        o.tol, o.tol_inf, o.max_iter, o.polish_tol = ZEROS['tol'], ZEROS['tol_inf'], ZEROS['max_iter'], ZEROS['polish_tol']
        seen.append((o.tol, o.tol_inf, o.max_iter, o.polish_tol, o.lazy_terminal, o.refine, o.polish))
        return o
    qp_backend._Options = raw
    try:
        qp = qp_backend.HipBatchedQP(ctrl.problem_data())
    finally:
        qp_backend._Options = real
    assert seen == [(0., -1., 0, -1e-4, 1, 1, 1)]
    same_records(qp.solve_batch(x0, fix), default, what='zero and negative option fields')
