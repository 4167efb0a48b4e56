"""The nodes of tests/test_gpu_narrow_stage.py: stages whose binaries are ALL fixed by the node take a narrow body in the register
factorisation (csrc/hmpc_kernel.hip, factor_reg, HMPC_NARROW_STAGE).  One list of nodes per problem
-- the cart-pole at N = 10 and N = 20, the cart-pole's leaves with the lazy terminal set switched off (the narrow body then runs
the last stage with the dense terminal block), a random MLD whose B has binary columns --, shared by the test and by
tests/golden/make_narrow_stage_parent.py, which writes the records of the commit before the narrow body to
tests/golden/narrow_stage_parent.npz.  Every problem is one that tests/jit_problems.py pre-warms: nothing compiles at test time.

Kinds of node (``kinds(fix, nub)`` names them): root; leaf (every stage fully fixed); a prefix of fully fixed stages, with and
without binaries fixed to one; stage 0 fully fixed only; a partially fixed stage right after the fully fixed ones.
"""
import os

import numpy as np

from helpers import make_controller, random_mld, _NoBackend

WAVES = ('1', '2', '4')
FIELDS = ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual')


def _nodes(T, nub, seed, leaves, p_one):
    """Row 0 the root.  (Few nodes: the records of the commit before are a committed file, tests/golden/narrow_stage_parent.npz.)"""
    rng = np.random.default_rng(seed)
    n = T * nub
    rows = [np.full(n, -1, np.int8)]
    def add(k, partial=0, ones=None, p=p_one):
        f = np.full(n, -1, np.int8)
        d = k * nub + partial
        f[:d] = (rng.random(d) < p).astype(np.int8) if ones is None else ones
        rows.append(f)
    for one in (0, 1):                                    # leaves: all zero, all one, drawn
        add(T, ones=one)
    for _ in range(leaves):
        add(T)
    f = np.zeros(n, np.int8); f[nub * (T // 2) + nub - 1] = 1   # a leaf with a single one
    rows.append(f)
    add(1, ones=0)                                        # stage 0 fully fixed only: to zero, to one, drawn
    add(1, ones=1)
    add(1, p=.5)
    for k in range(2, T, max(1, T // 3)):                 # prefixes of fully fixed stages: zeros, with ones
        add(k, ones=0)
        add(k, p=max(p_one, .3))
        add(k, partial=1 + (k % (nub - 1)) if nub > 1 else 0)   # ... and a partial stage right after them
    fix = np.unique(np.array(rows[1:]), axis=0)
    fix = np.vstack((rows[0][None], fix))
    assert len(fix) <= 64
    return fix


# the binaries of the N = 20 cart-pole's optimum from x0 = (0, 0, 1, 0): contact with the wall (a one) in stages 8 .. 16
_N20_INCUMBENT = np.array([[0, 0, 0, 0]] * 8 + [[0, 0, 0, 1]] * 2 + [[0, 0, 1, 1]] * 5 + [[0, 0, 1, 0]] * 2 + [[0, 0, 0, 0]] * 3, np.int8).ravel()


def _along(leaf, nub, stages, partial):
    """Nodes on the way to a leaf: its first k stages for k in ``stages``, each also with ``partial`` binaries of stage k."""
    rows = []
    for k in stages:
        for extra in (0, partial):
            f = np.full(leaf.size, -1, np.int8)
            f[:k * nub + extra] = leaf[:k * nub + extra]
            rows.append(f)
    return np.array(rows)


def kinds(fix, nub):
    """Counts of the kinds of node in a list (what the test asserts to be present)."""
    T = fix.shape[1] // nub
    st = fix.reshape(len(fix), T, nub)
    full = (st >= 0).all(axis=2)
    some = (st >= 0).any(axis=2)
    nfull = full.sum(axis=1)
    prefix = np.array([full[b, :nfull[b]].all() for b in range(len(fix))])
    return {'root': int((~some.any(axis=1)).sum()),
            'leaf': int((nfull == T).sum()),
            'fully fixed stage with a one': int(((st == 1).any(axis=2) & full).any(axis=1).sum()),
            'stage 0 only': int((prefix & (nfull == 1) & (some.sum(axis=1) == 1)).sum()),
            'partial stage after the fixed ones': int(np.sum([prefix[b] and 0 < nfull[b] < T and some[b, nfull[b]] and not full[b, nfull[b]]
                                                              for b in range(len(fix))]))}


def _cart_pole(T, x0, lazy=True, **kw):
    opts = {} if lazy else {'lazy_terminal': False}
    def make(backend):
        o = dict(opts, threads=8) if backend == 'oracle' else opts
        c = make_controller('cart_pole_with_walls', T=T, backend=backend, **o)
        return c, c.qp
    return dict(make=make, T=T, nub=4, x0=np.array(x0), efloor=None, **kw)


def _mld():
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    mld, objective, x0 = random_mld(nx=6, nuc=2, nub=3, seed=3)
    def make(backend):
        ctrl = HybridModelPredictiveController(mld, 12, objective, None, backend=_NoBackend())
        if backend == 'oracle':
            from oracle.oracle_qp import OracleBatchedQP
            return ctrl, OracleBatchedQP(ctrl.problem_data(), threads=8)
        from warm_start_hmpc_amd.qp_backend import HipBatchedQP
        return ctrl, HipBatchedQP(ctrl.problem_data())
    return dict(make=make, T=12, nub=3, x0=x0, efloor=1e-5)


def cases():
    out = {'n10': _cart_pole(10, [0., 0., .5, 0.]), 'n20': _cart_pole(20, [0., 0., 1., 0.]),
           'n10_dense_terminal': _cart_pole(10, [0., 0., .5, 0.], lazy=False), 'mld': _mld()}
    out['n10']['fix'] = _nodes(10, 4, 1, leaves=1, p_one=.05)
    out['n20']['fix'] = np.vstack((_nodes(20, 4, 2, leaves=0, p_one=.03), _N20_INCUMBENT[None], _along(_N20_INCUMBENT, 4, (9, 19), 2)))
    out['n20_dense_terminal'] = _cart_pole(20, [0., 0., 1., 0.], lazy=False)
    flipped = _N20_INCUMBENT.copy(); flipped[4 * 12 + 2] = 0
    out['n20_dense_terminal']['fix'] = np.array([_N20_INCUMBENT, flipped, np.ones(80, np.int8)])
    leaves = _nodes(10, 4, 3, leaves=1, p_one=.05)
    out['n10_dense_terminal']['fix'] = leaves[(leaves >= 0).all(axis=1)]          # (leaves only)
    ctrl, orc = out['mld']['make']('oracle')
    from helpers import dive_and_prefix_frontier
    dives = dive_and_prefix_frontier(orc, ctrl.mld, out['mld']['x0'], 12, 3)               # (on the way to feasible leaves: optimal nodes with ones)
    out['mld']['fix'] = np.vstack((_nodes(12, 3, 4, leaves=1, p_one=.3), dives[::27]))
    for c in out.values():
        assert len(c['fix']) <= 64
    return out


def kernel_records(qp, x0, fix):
    """{(waves, 'cold' | 'handdown'): records}: the cold kernel, and the hand-down instantiation with every optimal, polished node
    handed its own record."""
    out = {}
    for waves in WAVES:
        os.environ['HMPC_WAVES'] = waves
        try:
            a = qp.solve_batch(x0, fix)
            idx = np.where((a['status'] == 0) & (a['polished'] > 0), np.arange(len(fix)), -1).astype(np.int32)
            w = qp.solve_batch(x0, fix, warm=(a['primal'], a['dual'], idx))
        finally:
            del os.environ['HMPC_WAVES']
        out[(waves, 'cold')], out[(waves, 'handdown')] = a, w
    return out
