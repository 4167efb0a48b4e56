"""The problems and nodes of tests/test_gpu_factor_rows4.py: the stage block of the register factorisation (csrc/hmpc_kernel.hip,
factor_reg) lies on all four rows of 16 lanes of wave 0 (HMPC_FACTOR_ROWS4, the default); a build with -DHMPC_FACTOR_ROWS4=0 keeps
whole columns in lanes 0 .. nz-1 and is the reference every record is held to, bit for bit.

Problems: the two cart-pole shapes, <4,7,4> (nz = 11, no multiple of 4) and <4,4,2> (nz = 8), and a random MLD with nz = 15
(nx = 8, nu = 3 + 4), each at T = 2, T = 7 (the carve edge of DESIGN.md 7a) and T = 20.  Nodes per problem (a few dozen at most):
the root; stages with 1 .. nub-1 of their binaries fixed, the last of them to one (the constant direction mb / S.g of a partly
prescribed block), behind 0, T/2 and T-1 fully fixed stages; fully fixed stages (the narrow body) with and without ones, leaves
among them; on the cart-pole at T = 20 the nodes on the way to the incumbent, whose stages 8 .. 16 hold ones, on the random MLD the
nodes on the way to the leaf its relaxations lead to (optimal nodes whose fixed stages hold ones).  The cart-poles
run their nodes twice: with the lazy terminal set, and with the terminal set in every solve -- the dense block TG of the last stage.

``__graft_entry__.build()`` compiles the kernels of both builds of every problem without a GPU, so that the test loads them.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: F401  (puts the package on the path)
from helpers import load_fixture, make_controller, random_mld, _NoBackend
from narrow_stage_cases import _N20_INCUMBENT, _along

REFERENCE_FLAGS = '-DHMPC_FACTOR_ROWS4=0'
HORIZONS = (2, 7, 20)
SHAPES = ('walls_4_7_4', 'one_wall_4_4_2', 'mld_8_3_4')
NAMES = tuple('%s_T%d' % (s, T) for s in SHAPES for T in HORIZONS)
_FIXTURE = {'walls_4_7_4': 'cart_pole_with_walls', 'one_wall_4_4_2': 'cart_pole_one_wall'}


def nodes(T, nub, seed):
    rng = np.random.default_rng(seed)
    n = T * nub
    rows = [np.full(n, -1, np.int8)]                        # the root: no binary fixed
    def full(k, p):                                         # k fully fixed stages, ones with probability p
        f = np.full(n, -1, np.int8)
        f[:k * nub] = (rng.random(k * nub) < p).astype(np.int8)
        return f
    for k in sorted(set((0, T // 2, T - 1))):               # a partly fixed stage behind k fully fixed ones
        for m in range(1, nub):
            f = full(k, 0.)
            f[k * nub:k * nub + m] = 0
            f[k * nub + m - 1] = 1                          # ... its last fixed binary to one
            rows.append(f)
            f = full(k, 0.)
            f[k * nub:k * nub + m] = 0                      # ... and all to zero
            rows.append(f)
    for k in sorted(set((1, T // 2, T))):                   # fully fixed stages: zeros, drawn ones, a single one
        rows.append(full(k, 0.))
        rows.append(full(k, .15))
        f = full(k, 0.)
        f[(k - 1) * nub + nub - 1] = 1
        rows.append(f)
    fix = np.unique(np.array(rows[1:]), axis=0)
    return np.vstack((rows[0][None], fix))


def case(name):
    shape, T = name.rsplit('_T', 1)
    T = int(T)
    if shape in _FIXTURE:
        nub = int(load_fixture(_FIXTURE[shape])['nub'])
        x0 = np.array([0., 0., 1. if T == 20 else .5, 0.])
        fix = nodes(T, nub, 10 + T)
        if shape == 'walls_4_7_4' and T == 20:
            fix = np.vstack((fix, _N20_INCUMBENT[None], _along(_N20_INCUMBENT, 4, (9, 10, 16), 1), _along(_N20_INCUMBENT, 4, (10, 12), 3)))
        def make(backend, lazy=True):
            opts = {} if lazy else {'lazy_terminal': False}
            if backend == 'oracle':
                opts = dict(opts, threads=8)
            return make_controller(_FIXTURE[shape], T=T, backend=backend, **opts).qp
        def data():
            return make_controller(_FIXTURE[shape], T=T, backend=_NoBackend()).problem_data()
        lazies = (True, False)
    else:
        from warm_start_hmpc_amd.controller import HybridModelPredictiveController
        mld, objective, x0 = random_mld(nx=8, nuc=3, nub=4, seed=2)
        nub = 4
        fix = nodes(T, nub, 30 + T)
        def data():
            return HybridModelPredictiveController(mld, T, objective, None, backend=_NoBackend()).problem_data()
        def make(backend, lazy=True):
            if backend == 'oracle':
                from oracle.oracle_qp import OracleBatchedQP
                return OracleBatchedQP(data(), threads=8)
            from warm_start_hmpc_amd.qp_backend import HipBatchedQP
            return HipBatchedQP(data())
        lazies = (True,)
        # on the way to a leaf the relaxations lead to (helpers.dive_leaf): optimal nodes whose fixed stages hold ones
        from helpers import dive_leaf
        leaf = dive_leaf(make('oracle'), mld, x0, T)
        fix = np.vstack((fix, leaf[None], _along(leaf, nub, sorted(set((1, T // 2, T - 1))), 2)))
    assert len(fix) <= 48
    return dict(make=make, data=data, T=T, nub=nub, x0=x0, fix=fix, lazies=lazies)


class reference_build(object):
    """Inside: ``hmpc_create`` compiles (or finds in the cache) the kernels with whole columns per lane."""

    def __enter__(self):
        self.old = os.environ.get('HMPC_JIT_FLAGS')
        os.environ['HMPC_JIT_FLAGS'] = REFERENCE_FLAGS

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ['HMPC_JIT_FLAGS']
        else:
            os.environ['HMPC_JIT_FLAGS'] = self.old
