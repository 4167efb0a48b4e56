"""Shared test helpers: controllers built from the committed fixtures, synthetic frontiers."""
import os

import numpy as np

from warm_start_hmpc_amd.mld_system import MLDSystem
from warm_start_hmpc_amd.controller import HybridModelPredictiveController

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


class _NoBackend(object):
    """Placeholder so that a controller can be built before its backend exists."""


def lp_for(backend):
    """Batched LP solver that goes with a backend: the HIP kernel for the product path, the LP oracle otherwise."""
    if backend == 'hip':
        from warm_start_hmpc_amd.qp_backend import lp_solve_batch
    else:
        from oracle.oracle_lp import lp_solve_batch
    return lp_solve_batch


def load_fixture(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


def make_controller(name='cart_pole_with_walls', T=None, terminal=True, backend='oracle', **opts):
    """backend: 'oracle' (CPU, test infrastructure), 'hip' (the product path) or an object."""
    d = load_fixture(name)
    mld = MLDSystem([d['A'], d['B']], [d['F'], d['G'], d['h']], int(d['nub']))
    T = int(d['T']) if T is None else T
    term = [d['F_T'], d['h_T']] if terminal else None
    ctrl = HybridModelPredictiveController(mld, T, [d['Q'], d['R'], d['Q_T']], term, backend=_NoBackend(), lp=lp_for(backend))
    if backend == 'oracle':
        from oracle.oracle_qp import OracleBatchedQP
        ctrl.qp = OracleBatchedQP(ctrl.problem_data(), **opts)
    elif backend == 'hip':
        from warm_start_hmpc_amd.qp_backend import HipBatchedQP
        ctrl.qp = HipBatchedQP(ctrl.problem_data(), **opts)
    else:
        ctrl.qp = backend
    return ctrl


def long_head_parts():
    """Cart-pole with walls, N = 10, the committed terminal set listed twice -- (F_T, h_T) and (F_T, 1.5 h_T) -- so that the
    last stage has ncL = 28 + 2 x 102 = 232 rows (the warm-start shift's head of a row then exceeds one batch of 192).
    Returns (mld, T, objective, terminal set)."""
    d = load_fixture('cart_pole_with_walls')
    mld = MLDSystem([d['A'], d['B']], [d['F'], d['G'], d['h']], int(d['nub']))
    return mld, 10, [d['Q'], d['R'], d['Q_T']], [np.vstack((d['F_T'], d['F_T'])), np.concatenate((d['h_T'], 1.5 * d['h_T']))]


def random_prefix_frontier(T, nub, count, p_one=0.5, seed0=1000):
    """Synthetic frontier of SURVEY.md 8(d) C2: node k (seed seed0+k) fixes the first d binaries
    in (t, i) order, d ~ U{0..T*nub}, to Bernoulli(p_one) values; the rest are free (-1)."""
    fix = np.full((count, T * nub), -1, dtype=np.int8)
    for k in range(count):
        rng = np.random.default_rng(seed0 + k)
        d = int(rng.integers(0, T * nub + 1))
        fix[k, :d] = (rng.random(d) < p_one).astype(np.int8)
    return fix


def shallow_wide_family(name, T, count, width, depth=30, p_one=.15, seed=3):
    """Nodes with few fixed binaries (prefix length ~ U{0..depth-1}, Bernoulli(p_one) values) and one initial state per
    node, uniform over ``width`` of the state box: feasible-heavy, and -- for the one-wall system at N=40 -- home of the
    active sets whose multiplier steps need the second penalty level of the polish (terminal-set facets next to the
    state bounds they come from).  Returns (x0 [count, nx], fix [count, T nub])."""
    d = load_fixture(name)
    nub = int(d['nub'])
    rng = np.random.RandomState(seed)
    fix = np.full((count, T * nub), -1, np.int8)
    for k in range(count):
        dep = rng.randint(0, depth)
        fix[k, :dep] = rng.rand(dep) < p_one
    x0 = (rng.rand(count, d['A'].shape[0]) - .5) * 2 * d['x_max'] * width
    return x0, fix


def random_mld(nx=20, nuc=6, nub=8, seed=0):
    """Random MLD of SURVEY.md 8(d) C4 (a build decision, BASELINE.json leaves the rows open):
    stable A, box rows on x and uc, four big-M rows per binary."""
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((nx, nx))
    A = 0.95 * W / np.max(np.abs(np.linalg.eigvals(W)))
    nu = nuc + nub
    B = rng.standard_normal((nx, nu)) / np.sqrt(nx)
    B[:, nuc:] *= 0.5
    rows_F, rows_G, h = [], [], []
    for i in range(nx):
        for s in (1., -1.):
            f = np.zeros(nx); f[i] = s
            rows_F.append(f); rows_G.append(np.zeros(nu)); h.append(5.)
    for i in range(nuc):
        for s in (1., -1.):
            g = np.zeros(nu); g[i] = s
            rows_F.append(np.zeros(nx)); rows_G.append(g); h.append(1.)
    for j in range(nub):
        c = rng.standard_normal(nx); c /= np.linalg.norm(c)
        big = 5. * np.sum(np.abs(c))
        # b_j = 1 <=> c'x >= 0  (big-M), and the binary gates continuous input j % nuc
        g = np.zeros(nu); g[nuc + j] = -big
        rows_F.append(c.copy()); rows_G.append(g.copy()); h.append(0.)            #  c'x <= M b
        g = np.zeros(nu); g[nuc + j] = big
        rows_F.append(-c); rows_G.append(g.copy()); h.append(big)                 # -c'x <= M (1 - b)
        g = np.zeros(nu); g[j % nuc] = 1.; g[nuc + j] = -1.
        rows_F.append(np.zeros(nx)); rows_G.append(g.copy()); h.append(0.5)       #  uc <= .5 + b
        g = np.zeros(nu); g[j % nuc] = -1.; g[nuc + j] = -1.
        rows_F.append(np.zeros(nx)); rows_G.append(g.copy()); h.append(0.5)       # -uc <= .5 + b
    F, G, h = np.array(rows_F), np.array(rows_G), np.array(h)
    mld = MLDSystem([A, B], [F, G, h], nub)
    Q = np.eye(nx)
    R = np.hstack((np.eye(nuc), np.zeros((nuc, nub))))
    x0 = rng.uniform(-1, 1, nx) * 0.5
    return mld, [Q, R, Q.copy()], x0


def record_close(a, b, tol=1e-5):
    """Relative comparison of two result dicts from solve_batch (status exact, floats to tol)."""
    assert np.array_equal(a['status'], b['status']), (a['status'], b['status'])
    fin = np.isfinite(a['obj'])
    assert np.array_equal(fin, np.isfinite(b['obj']))
    np.testing.assert_allclose(a['obj'][fin], b['obj'][fin], rtol=tol, atol=tol * 1e-2)


def exercise_bounded_qp(ctrl):
    """The reference's one-node-at-a-time flow (controller.py:254-271 over bounded_qp.py:127-341) and the identities of
    test_bounded_qp.py:104-189 (Farkas signs, dual objective = -sum rhs * multiplier, strong duality) on a controller
    with T = 10 of the cart-pole-with-walls system, whatever its backend."""
    import pytest
    T, nub, nx = ctrl.T, ctrl.mld.nub, ctrl.mld.nx
    qp = ctrl.bounded_qp()
    with pytest.raises(RuntimeError, match='not solved'):
        qp.primal_objective()
    with pytest.raises(KeyError):
        qp.add_variables(3, lb=[0.] * 3)
    with pytest.raises(ValueError, match='right dimension'):
        qp.set_constraint_rhs('lam_0', np.zeros(nx + 1))
    with pytest.raises(ValueError, match='right dimension'):
        qp.set_constraint_rhs('no_such_family', np.zeros(2))
    assert qp.get_constraint_rhs('no_such_family').size == 0
    x0 = np.array([0., 0., .5, 0.])
    qp.set_constraint_rhs('lam_0', x0)
    ctrl._set_bound_binaries({(0, 0): 0., (0, 1): 0., (0, 2): 1.}, qp)
    np.testing.assert_array_equal(qp.get_constraint_rhs('nu_lb_0'), [-0., -0., -1., -0.])   # rhs of nu_lb is MINUS the bound
    np.testing.assert_array_equal(qp.get_constraint_rhs('nu_ub_0'), [0., 0., 1., 1.])
    np.testing.assert_array_equal(qp.get_constraint_rhs('mu_%d' % (T - 1)), ctrl.h_Tm1)

    def farkas_cost(q):       # - sum over ALL constraints of rhs * multiplier (bounded_qp.py:313-332)
        total = 0.
        for t in range(T + 1):
            total -= q.get_constraint_rhs('lam_%d' % t).dot(q.dual_optimizer('lam_%d' % t))
        for t in range(T):
            for fam in ('mu', 'nu_lb', 'nu_ub'):
                total -= q.get_constraint_rhs('%s_%d' % (fam, t)).dot(q.dual_optimizer('%s_%d' % (fam, t)))
        return total

    qp.optimize()                                                    # this node is infeasible (binary 2 on at time 0)
    assert np.isinf(qp.primal_objective()) and qp.primal_optimizer('x_1') is None
    assert qp.dual_objective() > 0 and abs(qp.dual_objective() - farkas_cost(qp)) < 1e-9 * (1 + qp.dual_objective())
    for t in range(T):
        for fam in ('mu', 'nu_lb', 'nu_ub'):
            assert np.all(qp.dual_optimizer('%s_%d' % (fam, t)) >= -1e-12)

    ctrl._set_bound_binaries({(0, i): 0. for i in range(nub)}, qp)  # feasible node
    with pytest.raises(RuntimeError, match='not solved'):          # editing a rhs invalidates the solution
        qp.dual_objective()
    qp.optimize()
    sol, _ = ctrl._solve_subproblem({(0, i): 0. for i in range(nub)}, x0)
    assert qp.primal_objective() == sol.primal.objective
    np.testing.assert_array_equal(qp.primal_optimizer('x_3'), sol.primal.variables['x'][3])
    np.testing.assert_array_equal(qp.dual_optimizer('mu_2'), sol.dual.variables['mu'][2])
    assert abs(qp.dual_objective() - qp.primal_objective()) < 1e-7                               # strong duality
    # dual objective of an optimal point from its multipliers: -1/4 (|rho|^2 + |sigma|^2) - sum rhs * multiplier
    quad = sum(np.sum(r ** 2) for r in sol.dual.variables['rho']) + sum(np.sum(s ** 2) for s in sol.dual.variables['sigma'])
    assert abs(-0.25 * quad + farkas_cost(qp) - qp.dual_objective()) < 1e-9
    qp.set_constraint_rhs('nu_ub_1', [.5, 1., 1., 1.])
    with pytest.raises(ValueError, match='free'):
        qp.optimize()


def real_tree_with_parents(ctrl, x0, leaves_too=False, **search):
    """Every node a cold-started branch and bound solves from x0, in solve order (and its leaves, on request), with the
    index of each node's parent among them (-1: the root, or a parent that is not in the list) -- the frontier of
    SURVEY.md 8(d) C2 "replayed real tree", and the shape in which the parent -> child hand-down (hmpc_warm) applies.
    Returns (fix int8 [n, T nub], parent int32 [n])."""
    seen, inner = [], ctrl.solve_frontier

    def recording(identifiers, x, *a, **k):
        seen.extend(ctrl._fix_vector(i) for i in identifiers)
        return inner(identifiers, x, *a, **k)
    ctrl.solve_frontier = recording
    try:
        _, leaves, _, _ = ctrl.feedforward(x0, printing_period=None, **search)
    finally:
        ctrl.solve_frontier = inner
    rows = seen + ([ctrl._fix_vector(l.identifier) for l in leaves] if leaves_too else [])
    fix = np.array(rows, dtype=np.int8)
    where = {}
    for i, f in enumerate(fix[:len(seen)]):
        where.setdefault(f.tobytes(), i)
    parent = np.full(len(fix), -1, dtype=np.int32)
    for i, f in enumerate(fix):
        d = int((f >= 0).sum())
        if d:
            g = f.copy()
            g[d - 1] = -1
            parent[i] = where.get(g.tobytes(), -1)
    return fix, parent


def dive_leaf(qp, mld, x0, T, feasible=False):
    """A dive to a leaf of a random MLD of random_mld: the binaries of stage t from the sign of c_j'x_t of the current relaxation,
    solved on ``qp`` (feasible: every relaxation on the way must be).  int8 [T nub]."""
    nx, nub, nuc = mld.nx, mld.nub, mld.nu - mld.nub
    Cj = np.array([mld.F[2 * nx + 2 * nuc + 4 * j] for j in range(nub)])
    leaf = np.full((1, T * nub), -1, np.int8)
    for t in range(T):
        r = qp.solve_batch(x0, leaf)
        assert r['status'][0] == 0 or not feasible
        leaf[0, t * nub:(t + 1) * nub] = (r['primal'][0][:(T + 1) * nx].reshape(T + 1, nx)[t] @ Cj.T >= 0)
    return leaf[0]


def dive_and_prefix_frontier(qp, mld, x0, T, seed, dives=96):
    """The frontier the random MLDs of helpers.random_mld are tested on (the kernels compiled per problem): 64 random prefixes
    (mostly infeasible) and ``dives`` prefixes of dive_leaf, every other one with one flipped binary.  int8 [64 + dives, T nub]."""
    nub = mld.nub
    leaf = dive_leaf(qp, mld, x0, T)[None]
    rng = np.random.default_rng(seed)
    fix = np.concatenate((random_prefix_frontier(T, nub, 64, p_one=0.3), np.full((dives, T * nub), -1, np.int8)))
    for k in range(65, 64 + dives):
        d = int(rng.integers(1, T * nub + 1))
        fix[k, :d] = leaf[0, :d]
        if k % 2 == 0:
            j = int(rng.integers(0, d))
            fix[k, j] = 1 - fix[k, j]
    return fix
