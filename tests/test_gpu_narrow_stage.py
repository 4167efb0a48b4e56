"""The narrow stage body of the register factorisation (csrc/hmpc_kernel.hip, factor_reg; HMPC_NARROW_STAGE): a stage whose
binaries are all fixed by the node forms, assembles and eliminates the rows of the states and the continuous inputs only.  Nothing
a solve returns may change by it.

On the nodes of tests/narrow_stage_cases.py -- root, leaves, prefixes of fully fixed stages with and without binaries fixed to one,
stage 0 alone, a partial stage right after the fixed ones; the cart-pole at N = 10 and N = 20, its leaves with the lazy terminal set
switched off (the narrow body runs the last stage with the dense terminal block), a random MLD whose B has binary columns -- at
1 / 2 / 4 waves per node, cold and hand-down instantiation, every record is held

  * to the CPU oracle at the tolerance of tests/test_gpu_parity.py (statuses equal node by node), and
  * to the record the commit before the narrow body returned for the same input (tests/golden/narrow_stage_parent.npz, written by
    tests/golden/make_narrow_stage_parent.py on that commit) at 1e-12 relative -- a fixture cannot promise bit equality across
    compiler builds.
"""
import numpy as np
import pytest

from helpers import load_fixture
from narrow_stage_cases import cases, kinds, kernel_records, FIELDS, WAVES

CASES = cases()
NAMES = tuple(CASES)
_ORACLE = {}


def _oracle(name):
    """The oracle's records of a problem's nodes: computed once, shared, left unchanged."""
    if name not in _ORACLE:
        c = CASES[name]
        ctrl, orc = c['make']('oracle')
        _ORACLE[name] = orc.solve_batch(c['x0'], c['fix'])
        for v in _ORACLE[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _ORACLE[name]


@pytest.mark.parametrize('name', NAMES)
def test_the_oracle_decides_every_node_and_every_kind_is_there(name):
    c = CASES[name]
    b = _oracle(name)
    assert len(c['fix']) <= 64
    assert np.all(b['status'] <= 1) and (b['status'] == 0).any() and (b['status'] == 1).any(), np.bincount(b['status'])
    k = kinds(c['fix'], c['nub'])
    assert k['leaf'] >= 1 and k['fully fixed stage with a one'] >= 1, k
    if not name.endswith('dense_terminal'):                     # (those: leaves only)
        assert k['root'] >= 1 and k['stage 0 only'] >= 1 and k['partial stage after the fixed ones'] >= 1, k
    if name in ('n20', 'mld', 'n20_dense_terminal'):            # an optimal node whose fully fixed stages hold a one: its constant direction counts
        st = c['fix'].reshape(len(c['fix']), c['T'], c['nub'])
        ones = ((st == 1).any(axis=2) & (st >= 0).all(axis=2)).any(axis=1)
        assert ((b['status'] == 0) & ones).any()
    g = load_fixture('narrow_stage_parent')
    assert np.array_equal(g[name + '/fix'], c['fix'])           # the committed records are those of these nodes


def _parent(g, name, waves, kind):
    """The parent commit's records (flags inside ``iters``, as the library writes them)."""
    key = '%s/%s/%s/' % (name, waves, kind)
    if kind == 'cold':
        return {k: g[key + k] for k in FIELDS}
    out = {k: np.array(v) for k, v in _parent(g, name, waves, 'cold').items()}
    rows = g[key + 'rows']
    for k in FIELDS:
        out[k][rows] = g[key + k]
    return out


def _close(a, b, what):
    """|a - b| <= 1e-12 max(1, largest entry of the row of b); NaN where b has NaN, infinities equal."""
    a, b = np.asarray(a, float).reshape(len(a), -1), np.asarray(b, float).reshape(len(b), -1)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), what
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]), what
    scale = np.maximum(1., np.max(np.where(fin, np.abs(b), 0.), axis=1, keepdims=True, initial=0.))
    dev = np.where(fin, np.abs(np.where(fin, a, 0.) - np.where(fin, b, 0.)), 0.) / scale
    print('%s: largest deviation from the parent commit %.2e' % (what, dev.max(initial=0.)))
    assert dev.max(initial=0.) <= 1e-12, (what, dev.max(), np.unravel_index(np.argmax(dev), dev.shape))


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_records_are_the_oracles_and_the_parent_commits(name):
    from test_gpu_parity import _compare
    c = CASES[name]
    ctrl, qp = c['make']('hip')
    assert qp.kernel_info() == (6, 6, 6), qp.kernel_info()      # the kernels compiled for the problem (pre-warmed: nothing compiles here)
    b = _oracle(name)
    g = load_fixture('narrow_stage_parent')
    recs = kernel_records(qp, c['x0'], c['fix'])
    assert sorted(recs) == sorted((w, k) for w in WAVES for k in ('cold', 'handdown'))
    for (waves, kind), a in recs.items():
        what = '%s, %s waves, %s' % (name, waves, kind)
        assert np.array_equal(a['status'], b['status']), (what, np.flatnonzero(a['status'] != b['status']))
        if kind == 'handdown':
            assert a['handed'].sum() >= 1, what                  # (the instantiation's own path ran)
        _compare(ctrl, a, b, c['T'], c['fix'], x0=c['x0'], efloor=c['efloor'])
        ref = _parent(g, name, waves, kind)
        assert np.array_equal(a['status'], ref['status']), what
        assert np.array_equal(a['iters'], ref['iters'] & 0xFFFF), what
        for flag, bit in (('polished', 16), ('weak', 17), ('handed', 18), ('second', 19), ('uncertified', 20)):
            assert np.array_equal(a[flag], (ref['iters'] >> bit) & 1), (what, flag)
        for k in ('obj', 'dual_obj', 'primal', 'dual'):
            _close(a[k], ref[k], what + ', ' + k)
