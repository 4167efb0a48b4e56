"""Every QP kernel's iterates held to the oracle's, iteration by iteration (the checks: tests/trajectory_checks.py).  ``max_iter = k``
with ``polish = 0`` in one pass returns the iterate after exactly k steps; the kernel's is compared with the oracle's, block by
block, to FACTOR times what the oracle itself moves when every entry of the problem data moves by 2^-52 relative.
The end-of-solve checks of the suite (statuses, records, certificates to 1e-8 .. 5e-6) see nothing of a kernel that loses digits
in its factorisation or its sweeps: the method corrects itself.  Its k-th iterate shows a relative defect of 1e-9 on every node.

Without a GPU: the oracle against its twins stays within the share of nodes that may be left out, its noise is finite and positive,
it mirrors itself with factor 1, and planted defects are refused by name.  Marked gpu: every kernel family on the workloads of
tests/test_solver_options.py, a defect planted on the device, and the build without the paired solve (-DHMPC_PAIR=0: the same
mathematics in another order) as the control that must pass.

FACTOR is measured, not chosen: the worst ratio of any kernel family to the oracle's own noise on an MI355X, times 4, rounded up to
a power of two and at most 4096 (the table of the run: profiles/iterate_trajectory.txt).  The ratio is against the
oracle and its twins, never against another kernel run; the margin is there for another box's code generation and for the
four-seed estimate of the noise (the maximum of four draws underestimates a tail)."""
import numpy as np
import pytest

from test_solver_options import _workload, _oracle, _copy, _env, FAMILIES
from trajectory_checks import (BLOCKS, EXCLUDED, UNDECIDED, columns, blocks, deviation, ulp_twins, off_by, noise, left_out, left_out_cap, ratios,
                               mirrors, ratios_line)
from oracle.oracle_qp import OracleBatchedQP

FACTOR = 64.                                                         # worst ratio measured: 10.1 (mld10, streaming form, k = 8); x 4 = 40.4
KS = (1, 2, 3, 4, 6, 8, 10, 12)
WORKLOADS = ('walls10', 'one_wall20', 'mld8', 'mld10')
DEFECT = 1e-9                                                        # the planted defect: B off by this, relative
_TWINS, _DATA, _PLANTED = {}, {}, {}
TABLE = {}


def _options(k):
    return dict(polish=0, lazy_terminal=0, max_iter=k)


def _ref(name, k):
    return _oracle(name, **_options(k))


def _twins(name, k):
    """The oracle's records on the four ulp twins of a workload's data after k iterations (computed once, shared, never written to)."""
    if (name, k) not in _TWINS:
        ctrl, x0, fix, _ = _workload(name)
        if name not in _DATA:
            _DATA[name] = ulp_twins(ctrl.problem_data())
        _TWINS[name, k] = [OracleBatchedQP(data, threads=8, **_options(k)).solve_batch(x0, fix) for data in _DATA[name]]
    return _TWINS[name, k]


def _planted(name, k):
    """The oracle's records on data whose B is off by DEFECT."""
    if (name, k) not in _PLANTED:
        ctrl, x0, fix, _ = _workload(name)
        _PLANTED[name, k] = OracleBatchedQP(off_by(ctrl.problem_data(), 'B', DEFECT), threads=8, **_options(k)).solve_batch(x0, fix)
    return _PLANTED[name, k]


def _ks(name):
    """1, 2, 3, 4, 6, 8, 10, and 12 where at least 8 nodes are still undecided on the oracle."""
    return tuple(k for k in KS if k < 12 or (_ref(name, k)['status'] == UNDECIDED).sum() >= 8)


def _refused(name, rec, k):
    """How many of the nodes compared lie over the bound at FACTOR, and how many are compared."""
    ctrl, _, fix, _ = _workload(name)
    rows, ratio, _, _ = ratios(ctrl, fix, rec, _ref(name, k), _twins(name, k))
    return int((~(ratio <= FACTOR)).sum()), len(rows)


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', WORKLOADS)
def test_the_oracle_beside_its_twins(name):
    ctrl, x0, fix, _ = _workload(name)
    assert _ks(name) == KS                                            # (k = 12 leaves 18 .. 42 nodes undecided on the four workloads)
    for k in _ks(name):
        ref, twins = _ref(name, k), _twins(name, k)
        und = ref['status'] == UNDECIDED
        assert und.all() if k <= 4 else und.sum() >= 8, (name, k, und.sum())
        # the share that may be left out is a condition on the workloads, not a measurement: the oracle itself stays within it
        assert left_out([ref] + twins).size <= left_out_cap(len(fix)), (name, k)
        nz = noise(ctrl, fix, ref, twins)
        seen = np.isfinite(nz)
        assert seen.sum() >= 8 and np.all(nz[seen] > 0.) and np.all(nz[seen] < 1e-7), (name, k, nz[seen].min(), nz[seen].max())
        assert not np.any(seen & ~und)
        assert mirrors(ctrl, fix, ref, ref, twins, k, 1., what='%s oracle' % name) == 0.
        # a twin in the kernel's place, beside the oracle and the three others: the oracle's own arithmetic on data one rounding away
        # passes as a kernel has to (measured: at most 6.5 x the noise the other three show), and is not the oracle's record
        for i in range(len(twins)):
            assert 0. < mirrors(ctrl, fix, twins[i], ref, twins[:i] + twins[i + 1:], k, FACTOR, what='%s twin %d' % (name, i))


def test_the_twins_move_every_entry_by_2_to_the_minus_52_and_nothing_else():
    data = _workload('mld10')[0].problem_data()
    twins = ulp_twins(data)
    assert len(twins) == 4
    arrays = [k for k, v in data.items() if isinstance(v, np.ndarray) and v.dtype == np.float64]
    assert set(('A', 'B', 'F', 'G', 'h', 'F_Tm1', 'G_Tm1', 'h_Tm1', 'Q', 'R', 'Q_T')) <= set(arrays)
    for twin in twins:
        assert set(twin) == set(data)
        for k, v in data.items():
            if k not in arrays:
                assert twin[k] is v or twin[k] == v
                continue
            assert twin[k].shape == v.shape and twin[k].dtype == v.dtype and np.array_equal(twin[k] == 0., v == 0.)
            assert np.all(np.abs(twin[k] - v) <= 2. ** -51 * np.abs(v))      # (2^-52 |v| rounded to the grid of v: one or two of its units)
        assert sum(int((twin[k] != data[k]).sum()) for k in arrays) > 0.3 * sum(int((data[k] != 0.).sum()) for k in arrays)
    assert any(not np.array_equal(twins[0][k], twins[1][k]) for k in arrays)
    for a, b in zip(twins, ulp_twins(data)):                          # (seeded: the same twins every time)
        assert all(np.array_equal(a[k], b[k]) for k in arrays)


@pytest.mark.parametrize('name', ['walls10', 'mld8'])
def test_blocks_partition_both_rows(name):
    ctrl, x0, fix, _ = _workload(name)
    layout, cut, B = ctrl.layout, columns(ctrl.layout), len(fix)
    for row, width in (('primal', layout.n_primal), ('dual', layout.n_dual)):
        got = np.concatenate([idx for r, idx in cut.values() if r == row])
        assert np.array_equal(np.sort(got), np.arange(width)), row
    assert not EXCLUDED and set(BLOCKS) == set(cut) - set(('nu_lb', 'nu_ub')) | set(('nu_free', 'nu_fixed'))
    # a record whose every column holds its own number: each shows up in exactly one block -- the two bound columns of a binary in
    # nu_free where the node leaves it free, as their difference in nu_fixed where it fixes it
    rec = dict(primal=np.tile(np.arange(1., layout.n_primal + 1.), (B, 1)), dual=np.tile(np.arange(1., layout.n_dual + 1.), (B, 1)))
    got = blocks(ctrl, rec, fix)
    assert tuple(got) == BLOCKS
    lb, ub = cut['nu_lb'][1] + 1., cut['nu_ub'][1] + 1.
    assert (fix < 0).any() and (fix >= 0).any() and np.all(ub - lb != 0.)
    for i in range(B):
        free = fix[i] < 0
        for k in ('x', 'u', 'lam', 'mu', 'rho', 'sig'):
            assert np.array_equal(got[k][i], cut[k][1] + 1.)
        assert np.array_equal(got['nu_free'][i], np.concatenate((np.where(free, lb, 0.), np.where(free, ub, 0.))))
        assert np.array_equal(got['nu_fixed'][i], np.where(free, 0., ub - lb))
    # the split of a fixed binary's multiplier is a convention of the record: both columns moved by the same amount, nothing deviates;
    # the bound columns of a free binary are two multipliers, and moving them does
    ref = _ref(name, 2)
    node = int(np.flatnonzero((fix >= 0).any(axis=1) & (fix < 0).any(axis=1))[0])
    fixed, free = np.flatnonzero(fix[node] >= 0)[0], np.flatnonzero(fix[node] < 0)[0]
    moved = _copy(ref)
    moved['dual'][node, [cut['nu_lb'][1][fixed], cut['nu_ub'][1][fixed]]] += 1.
    per, worst = deviation(blocks(ctrl, moved, fix), blocks(ctrl, ref, fix), [node])
    assert worst[0] <= 4 * 2. ** -52 and per['nu_free'][0] == 0.
    moved['dual'][node, [cut['nu_lb'][1][free], cut['nu_ub'][1][free]]] += 1.
    per, worst = deviation(blocks(ctrl, moved, fix), blocks(ctrl, ref, fix), [node])
    assert per['nu_free'][0] > .1 and per['nu_fixed'][0] <= 4 * 2. ** -52 and worst[0] == per['nu_free'][0]
    # an entry that is no number on one side alone is an infinite deviation
    moved = _copy(ref)
    moved['primal'][node, 3] = np.nan
    assert deviation(blocks(ctrl, moved, fix), blocks(ctrl, ref, fix), [node])[0]['x'][0] == np.inf


@pytest.mark.parametrize('name', WORKLOADS)
@pytest.mark.parametrize('k', [1, 2])
def test_a_relative_defect_of_1e_9_is_refused_on_nine_nodes_in_ten(name, k):
    # (a) the oracle on data whose B is off by 1e-9 relative: invisible to every end-of-solve check of the suite (1e-8 at the best)
    ctrl, x0, fix, _ = _workload(name)
    rec = _planted(name, k)
    assert np.all(rec['status'] == UNDECIDED)
    with pytest.raises(AssertionError, match='^mirrors: %s planted k %d node \\d+ block ' % (name, k)):
        mirrors(ctrl, fix, rec, _ref(name, k), _twins(name, k), k, FACTOR, what='%s planted' % name)
    over, compared = _refused(name, rec, k)
    rows, ratio, _, _ = ratios(ctrl, fix, rec, _ref(name, k), _twins(name, k))
    print('%s k %d: planted defect, ratio min / 10 %% / median: %.3g / %.3g / %.3g' % (name, k, ratio.min(), np.sort(ratio)[len(ratio) // 10], np.median(ratio)))
    assert compared == len(fix) and over >= 0.9 * compared


def test_planted_defects_in_records_are_refused_by_name():
    name, k = 'walls10', 4
    ctrl, x0, fix, _ = _workload(name)
    layout, cut = ctrl.layout, columns(ctrl.layout)
    ref, twins = _ref(name, k), _twins(name, k)
    factor = FACTOR
    args = dict(k=k, factor=factor, what='%s planted' % name)
    assert mirrors(ctrl, fix, _copy(ref), ref, twins, **args) == 0.
    # (b) an iteration word that says k + 1 (the flag bits above bit 16 are not the count)
    rec = _copy(ref)
    rec['iters'] = rec['iters'] | (1 << 19)
    mirrors(ctrl, fix, rec, ref, twins, **args)
    rec['iters'][7] += 1
    with pytest.raises(AssertionError, match='^mirrors: walls10 planted k 4 node 7: undecided after 5 iterations, not 4'):
        mirrors(ctrl, fix, rec, ref, twins, **args)
    # (c) one stage's u rows exchanged with the next stage's
    rec = _copy(ref)
    u, nu = cut['u'][1], layout.nu
    rec['primal'][5, u[3 * nu:4 * nu]], rec['primal'][5, u[4 * nu:5 * nu]] = ref['primal'][5, u[4 * nu:5 * nu]], ref['primal'][5, u[3 * nu:4 * nu]]
    with pytest.raises(AssertionError, match='^mirrors: walls10 planted k 4 node 5 block u: '):
        mirrors(ctrl, fix, rec, ref, twins, **args)
    # (d) a lam row of one node zeroed
    rec = _copy(ref)
    row = cut['lam'][1][2 * layout.nx:3 * layout.nx]
    assert np.abs(ref['dual'][9, row]).max() > 1e-6
    rec['dual'][9, row] = 0.
    with pytest.raises(AssertionError, match='^mirrors: walls10 planted k 4 node 9 block lam: '):
        mirrors(ctrl, fix, rec, ref, twins, **args)
    # (e) a node decided in rec with another status than in ref
    k = 10
    ref, twins = _ref(name, k), _twins(name, k)
    decided = np.flatnonzero(ref['status'] <= 1)
    assert decided.size >= 8
    rec = _copy(ref)
    rec['status'][decided[0]] = 1 - ref['status'][decided[0]]
    with pytest.raises(AssertionError, match='^mirrors: walls10 planted k 10 node %d: decided with status %d, the reference with %d'
                       % (decided[0], 1 - ref['status'][decided[0]], ref['status'][decided[0]])):
        mirrors(ctrl, fix, rec, ref, twins, k, factor, what='%s planted' % name)
    # ... and more nodes decided on one side alone than may be left out
    rec = _copy(ref)
    rec['status'][np.flatnonzero(ref['status'] == UNDECIDED)[:left_out_cap(len(fix)) + 1]] = 0
    with pytest.raises(AssertionError, match='^mirrors: walls10 planted k 10: %d nodes decided on one side' % (left_out_cap(len(fix)) + 1)):
        mirrors(ctrl, fix, rec, ref, twins, k, factor, what='%s planted' % name)
    rec = _copy(ref)
    rec['status'][np.flatnonzero(ref['status'] == UNDECIDED)[:left_out_cap(len(fix))]] = 0
    mirrors(ctrl, fix, rec, ref, twins, k, factor, what='%s planted' % name)
    assert left_out_cap(144) == 4 and left_out_cap(20) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _waves(n, kinds, **env):
    return (dict(env, HMPC_WAVES=n), kinds)


# problem: {family: (environment that selects the kernels, the kinds hmpc_kernel_info names -- None: compiled for the problem, >= 4)}
LEGS = {
    'walls10': {f: FAMILIES[f] for f in ('default', 'shipped_w1', 'shipped_w2', 'shipped_w4', 'generic', 'streaming')},
    'one_wall20': {f: FAMILIES[f] for f in ('default', 'shipped_w2', 'shipped_w4')},        # (the shipped <4, 4, 2> kernels: two and four waves)
    # nz = 15: the register kernel compiled for the shape
    'mld8': {'register_w%d' % n: _waves(n, (6, 6, 6)) for n in (1, 2, 4)},
    # nz = 18: beyond the static row map -- the run-time-sized kernel (its matrix-core stage matrix, and at four waves factor_tiles),
    # compiled with the problem's sizes, as shipped, and in its streaming form
    'mld10': dict([('sized_w%d' % n, _waves(n, (4, 4, 4))) for n in (1, 2, 4)] + [('generic_w%d' % n, _waves(n, (0, 0, 0), HMPC_JIT_SIZED=0)) for n in (1, 2, 4)]
                  + [('streaming', FAMILIES['streaming'])]),
}


def _kernel(name, env, kinds, k, data=None):
    """The records of a workload after k iterations of the kernels ``env`` selects: a handle of its own, no second opinion of another
    kernel (HMPC_JIT_SELFCHECK=0: a batch that is undecided by construction would be solved again by the shipped kernel, and the
    record would no longer tell which binary wrote it)."""
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    ctrl, x0, fix, _ = _workload(name)
    with _env(**dict(env, HMPC_JIT_SELFCHECK=0)):
        qp = HipBatchedQP(ctrl.problem_data() if data is None else data, **_options(k))
        assert qp.kernel_info() == kinds if kinds else min(qp.kernel_info()) >= 4, (name, env, qp.kernel_info())
        rec = qp.solve_batch(x0, fix)
        assert qp.jit_stats()[0] == 0 and (qp.kernel_info() == kinds if kinds else min(qp.kernel_info()) >= 4), (name, env, qp.jit_stats(), qp.kernel_info())
    return rec


@pytest.fixture(scope='module')
def report():
    yield
    if TABLE:
        print('\n' + ratios_line(TABLE))


def _hold(name, family, env, kinds):
    ctrl, x0, fix, _ = _workload(name)
    row = TABLE.setdefault((name, family), {})
    failed = []
    for k in _ks(name):
        rec = _kernel(name, env, kinds, k)
        try:
            row[k] = mirrors(ctrl, fix, rec, _ref(name, k), _twins(name, k), k, FACTOR, what='%s %s' % (name, family))
        except AssertionError as exc:                                     # (every k is run: the table shows where a defect begins)
            row[k] = float(ratios(ctrl, fix, rec, _ref(name, k), _twins(name, k))[1].max(initial=0.))
            failed.append(str(exc))
    print('%s %s: %s' % (name, family, ' '.join('%d %.3g' % kv for kv in sorted(row.items()))))
    assert not failed, '\n'.join(failed)


@pytest.mark.gpu
@pytest.mark.parametrize('name,family', [(n, f) for n in LEGS for f in LEGS[n]])
def test_every_kernel_mirrors_the_oracle_iteration_by_iteration(report, name, family):
    _hold(name, family, *LEGS[name][family])


@pytest.mark.gpu
def test_the_build_without_the_paired_solve_mirrors_the_oracle_too(report):
    # the negative control: the two solves of an iteration one after the other instead of in one pair of sweeps -- the same
    # mathematics in another order, which a factor that asked for bit-equality would refuse
    from jit_problems import WITHOUT_PAIR                               # (pre-built with the other kernels of the suite: nothing compiles here)
    _hold('walls10', 'default %s' % WITHOUT_PAIR, dict(HMPC_JIT_FLAGS=WITHOUT_PAIR), None)


@pytest.mark.gpu
@pytest.mark.parametrize('name,env,kinds', [('walls10',) + FAMILIES['shipped_w1'], ('mld10', dict(HMPC_JIT=0), (0, 0, 0))])
def test_a_relative_defect_of_1e_9_on_the_device_is_refused(name, env, kinds):
    # kernels that need no compilation for other data: created on data whose B is off by 1e-9 relative, compared with the oracle on
    # the true data
    ctrl, x0, fix, _ = _workload(name)
    assert np.isfinite(FACTOR)
    for k in (1, 2):
        rec = _kernel(name, env, kinds, k, data=off_by(ctrl.problem_data(), 'B', DEFECT))
        with pytest.raises(AssertionError, match='^mirrors: %s planted k %d node \\d+ block ' % (name, k)):
            mirrors(ctrl, fix, rec, _ref(name, k), _twins(name, k), k, FACTOR, what='%s planted' % name)
        over, compared = _refused(name, rec, k)
        print('%s k %d: %d of %d nodes refused' % (name, k, over, compared))
        assert compared == len(fix) and over >= 0.9 * compared
