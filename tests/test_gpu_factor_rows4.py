"""The stage block of the register factorisation on all four rows of 16 lanes (csrc/hmpc_kernel.hip, factor_reg;
HMPC_FACTOR_ROWS4): nothing a solve returns may change by it, not in the last bit.

On the problems and nodes of tests/factor_rows4_cases.py -- <4,7,4>, <4,4,2> and a random MLD with nz = 15, each at T = 2, 7 and 20;
no binary fixed, partly fixed stages with a one, fully fixed stages, the dense terminal block -- at 1 / 2 / 4 waves per node, cold and
hand-down instantiation, every record is held

  * BIT FOR BIT to the record of the build with -DHMPC_FACTOR_ROWS4=0 (whole columns per lane: the kernels of the commit before),
    compiled from the same tree -- objectives, primal and dual rows as bytes, statuses and ``iters`` words (flags included) exactly;
  * to the CPU oracle: statuses node by node and helpers.record_close.
"""
import numpy as np
import pytest

from helpers import record_close
from factor_rows4_cases import NAMES, case, reference_build
from narrow_stage_cases import kernel_records, WAVES

FLOATS = ('obj', 'dual_obj', 'primal', 'dual')
WORDS = ('status', 'iters', 'polished', 'weak', 'handed', 'second', 'uncertified')


def test_the_nodes_cover_the_stage_kinds():
    for name in NAMES:
        c = case(name)
        st = c['fix'].reshape(len(c['fix']), c['T'], c['nub'])
        nfixed = (st >= 0).sum(axis=2)
        ones = (st == 1).any(axis=2)
        assert (nfixed == 0).all(axis=1).any(), name                                  # a node with no binary fixed
        for m in range(1, c['nub']):                                                  # m of the stage's binaries fixed, one of them to one
            assert ((nfixed == m) & ones).any(), (name, m)
        assert ((nfixed == c['nub']) & ones).any() and ((nfixed == c['nub']) & ~ones).any(), name   # fully fixed stages, with and without a one
        assert (nfixed == c['nub']).all(axis=1).any(), name                           # a leaf
        assert (nfixed[:, -1] == c['nub']).any() and (nfixed[:, -1] == 0).any(), name  # the last stage (terminal block) in both bodies
        assert len(c['fix']) <= 48


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_records_keep_every_bit_and_are_the_oracles(name):
    c = case(name)
    for lazy in c['lazies']:
        qp = c['make']('hip', lazy)
        with reference_build():
            ref = c['make']('hip', lazy)
        assert qp.kernel_info() == ref.kernel_info() == (6, 6, 6), (qp.kernel_info(), ref.kernel_info())   # register kernels compiled for the problem
        b = c['make']('oracle', lazy).solve_batch(c['x0'], c['fix'])
        assert np.all(b['status'] <= 1), np.bincount(b['status'])
        new, old = kernel_records(qp, c['x0'], c['fix']), kernel_records(ref, c['x0'], c['fix'])
        assert sorted(new) == sorted(old) == sorted((w, k) for w in WAVES for k in ('cold', 'handdown'))
        assert qp.jit_stats()[0] == 0 and ref.jit_stats()[0] == 0                     # no compiled kernel dropped: these kernels ran
        for key, a in new.items():
            what = '%s, lazy terminal set %s, %s waves, %s' % ((name, lazy) + key)
            r = old[key]
            for k in WORDS:
                assert np.array_equal(a[k], r[k]), (what, k, np.flatnonzero(a[k] != r[k]))
            for k in FLOATS:
                same = np.ascontiguousarray(a[k]).view(np.uint64) == np.ascontiguousarray(r[k]).view(np.uint64)
                assert same.all(), (what, k, 'first differing entries', np.argwhere(~same)[:4], float(np.nanmax(np.abs(a[k] - r[k]))))
            assert np.array_equal(a['status'], b['status']), (what, np.flatnonzero(a['status'] != b['status']))
            record_close(a, b)
