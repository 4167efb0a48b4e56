"""Records of solves with a parent -> child hand-down (``hmpc_warm``): written, repeatable, independent of the company a node is
solved in, certified, and the same bounds for the children -- through the C ABI, on every kernel family.

Why: the multipliers of a handed record become the children's bounds (csrc/hmpc_branch.h) and, through the warm-start shift, the
next step's.  Until this file the result of a solve with a hand-down depended on what the process did before (figures:
profiles/handdown_records.txt): objective, status, iters word and primal row to the bit, but the nu_lb / nu_ub entries of the
binaries a node FIXES, of nodes whose handed set verified, 0 in one launch and the multiplier (30 .. 60) in the next, the dual
objective with them where a binary is fixed to one, the certificate's stationarity at order one.  Nothing was unwritten (with
fills of +0. and -0. step 6 of tests/test_gpu_staging.py had read it so).  The cause: a handed node enters the polish without an
interior-point pass, and the hand-down writes the multiplier-step slot R.dz of the rows of its set only.  The slots of the rows
that take no part -- the bounds of the binaries the node fixes -- hold what the previous node or launch left in the register;
the polish multiplied them by D = 0 for the right-hand side, and where the register held no number the NaN stayed in S.e, missed
the sweeps (a fixed binary is prescribed), reached the fixed binaries' multipliers through their stationarity row, and
write_record splits a NaN by sign into two zeros.  Solves alone leave numbers in those registers: with only another cold batch
between the launches all 18 cases were bit-equal on the code before; with the certificates and the children of that batch's
records in between (NaN primal rows of infeasible records) 10 of 18 failed.  The hand-down instantiation now takes 0 for a row
with D = 0 instead of 0 * the slot (csrc/hmpc_kernel.hip, the right-hand side of the constant direction).

Batches (shapes the suite compiles anyway):
  A  cart-pole with walls, T = 10, x0 = (0, 0, .5, 0): 65 children of optimal nodes of a 300-node prefix frontier, every third
     handed its parent's record (step 6 of tests/test_gpu_staging.py).  22 handed: verified and fallen back to the cold start.
  B  the same system, T = 20, x0 = (0, 0, 1, 0): the tree a cold branch and bound solves (160 nodes), every node with a polished
     optimal parent handed.  159 handed: verified, fallen back, infeasible.
  C  T = 10, x0 = (0, 0, .5, 0): the tree a cold branch and bound solves (80 nodes), handed in the same way.  It supplies the
     kind neither A nor B has: a node whose parent's optimum lies on terminal-set facets, which is first tried WITH the terminal
     rows (HMPC_ITERS_TERMINAL | HMPC_ITERS_HANDED).  The trees at T = 20 and T = 40 from x0 = (0, 0, 1, 0) hold no such node
     (checked with the oracle: their only nodes that need the terminal rows are infeasible and hand nothing down).
The kinds are counted from the ``iters`` word and asserted per batch; the oracle's records of the same hand-down (which flag a
verified hand-down as polished == 64) are counted in the same way first.

Kernels: the register kernels at 1, 2 and 4 waves per node, the run-time-sized kernel, its streaming form, and the default once
more without the first-use check and the second opinion (what the compiled kernel itself returns).

What is held, for every array of the record and every node, handed or not:
  written      launches of the device-pointer entry into outputs filled with two different quiet-NaN payloads (integers: two
               non-zero words); an entry is unwritten iff its bits equal its fill.
  repeatable   three launches of the same batch; before each, on the same handle, a DIFFERENT cold batch (the 300-node frontier at
               0.8 x0) with the certificates and the children of its records -- they leave other nodes' LDS and registers
               behind, NaN primal rows of infeasible records among them --: all six arrays bit-equal, and bit-equal to the
               host-pointer entry.
  company      the handed nodes alone, with their parents' rows gathered and the index renumbered, and once more in reversed
               order: the same records to the bit.
  certified    every one of these runs holds its own KKT / Farkas certificates (tests/certificates.py; the margins come from the
               oracle's records of the same hand-down, no tolerance is introduced here).
  downstream   hmpc_branch_batch on the handed records of the first and of the third run: the same children to the bit.
The figures (unwritten entries and rows, differing entries and rows, largest difference, per block of the dual row) are printed;
profiles/handdown_records.txt keeps those of the code before and after.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import branch_reference as br
import search_reference as sr
from certificates import assert_certified, record_from_device
from helpers import make_controller, random_prefix_frontier, real_tree_with_parents
from test_gpu_staging import _bits_differ, _to

pytestmark = pytest.mark.gpu
ARRAYS = ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual')
# two quiet NaNs with payloads of their own (the kernel writes 0x7ff8000000000000 into the primal row of an infeasible node)
NAN_FILL = (0x7ff80000dead0001, 0x7ff80000beef0002)
INT_FILL = (0x5a5a5a5a, 0x3c3c3c3c)
assert 0x7ff8000000000000 not in NAN_FILL and NAN_FILL[0] != NAN_FILL[1] and 0 not in INT_FILL and INT_FILL[0] != INT_FILL[1]
KINDS = ('verified', 'fallen back', 'terminal rows', 'infeasible')
BATCHES = {'A': (10, np.array([0., 0., .5, 0.]), ('verified', 'fallen back')),
           'B': (20, np.array([0., 0., 1., 0.]), ('verified', 'fallen back', 'infeasible')),
           'C': (10, np.array([0., 0., .5, 0.]), KINDS)}
# name: (environment while the handle is created, environment while it solves) -- as tests/test_gpu_parity.py sets them
KERNELS = {'register-1-wave': ({}, {'HMPC_WAVES': '1'}), 'register-2-waves': ({}, {'HMPC_WAVES': '2'}), 'register-4-waves': ({}, {'HMPC_WAVES': '4'}),
           'run-time-sized': ({'HMPC_FORCE_GENERIC': '1'}, {}), 'streaming': ({'HMPC_FORCE_BIG': '1'}, {}),
           'no-selfcheck': ({'HMPC_JIT_SELFCHECK': '0'}, {})}
_HANDLES = {}


@contextlib.contextmanager
def _env(values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _handle(kernel, T):
    if (kernel, T) not in _HANDLES:
        with _env(KERNELS[kernel][0]):
            _HANDLES[kernel, T] = make_controller('cart_pole_with_walls', T=T, backend='hip')
    return _HANDLES[kernel, T]


def _kinds(index, status, iters_word, verified):
    """Number of handed nodes of each kind of KINDS (a node may be of two: the terminal rows and verified or fallen back)."""
    h = index >= 0
    return {'verified': int((h & verified).sum()), 'fallen back': int((h & (status == 0) & ~verified & ((iters_word & 0xFFFF) > 0)).sum()),
            'terminal rows': int((h & ((iters_word & br.TERMINAL_BIT) != 0)).sum()), 'infeasible': int((h & (status == 1)).sum())}


@functools.lru_cache(maxsize=None)
def _batch(name):
    """The batch and the oracle's records of it, computed once: dict x0, fix [B], index [B] (row of the parent in ``table_fix`` or
    -1), table_fix (the nodes whose cold records are the parents' rows), dirty (the other batch: 300 prefixes, solved at 0.8 x0),
    cold_status (the oracle's, of table_fix), ref (the oracle's records of the hand-down), orc."""
    T, x0, kinds = BATCHES[name]
    orc = make_controller('cart_pole_with_walls', T=T, backend='oracle', threads=8)
    dirty = random_prefix_frontier(T, orc.mld.nub, 300, p_one=0.1)
    dirty[0, :] = -1
    if name == 'A':
        table_fix = dirty
        cold = orc.qp.solve_batch(x0, table_fix)
        parents = np.flatnonzero((table_fix < 0).any(axis=1) & (cold['status'] == 0))[:65]
        assert len(parents) == 65
        fix = table_fix[parents].copy()
        fix[np.arange(65), (fix < 0).argmax(axis=1)] = 0
        index = np.where(np.arange(65) % 3 == 0, parents, -1).astype(np.int32)
    else:
        fix, parent = real_tree_with_parents(orc, x0)
        table_fix = fix
        cold = orc.qp.solve_batch(x0, fix)
        ok = (parent >= 0) & (cold['status'][np.maximum(parent, 0)] == 0) & (cold['polished'][np.maximum(parent, 0)] > 0)
        index = np.where(ok, parent, -1).astype(np.int32)
    assert np.all(cold['polished'][index[index >= 0]] > 0)                       # (only polished optimal records may be handed down)
    ref = orc.qp.solve_batch(x0, fix, warm=(cold['primal'], cold['dual'], index))
    seen = _kinds(index, ref['status'], br.iters_word(ref), ref['polished'] == 64)
    assert {k for k in KINDS if seen[k]} == set(kinds), (name, 'kinds of handed nodes on the oracle', seen)
    return dict(T=T, x0=x0, fix=fix, index=index, table_fix=table_fix, dirty=dirty, cold_status=cold['status'], ref=ref, orc=orc)


def _launch(qp, x0, fix, warm=None, which=0):
    """One launch of the device-pointer entry into outputs that hold fill ``which``: (records, {array: mask of the entries left unwritten})."""
    import torch
    B = len(fix)
    shapes = dict(obj=(B,), dual_obj=(B,), status=(B,), iters=(B,), primal=(B, qp.n_primal), dual=(B, qp.n_dual))
    fill = {k: (np.full(s, INT_FILL[which], np.uint32).view(np.int32) if k in ('status', 'iters') else np.full(s, NAN_FILL[which], np.uint64).view(np.float64))
            for k, s in shapes.items()}
    out = {k: _to(v) for k, v in fill.items()}
    qp.solve_batch_device(_to(x0), _to(fix), out, warm=warm)
    torch.cuda.synchronize()
    rec = {k: v.cpu().numpy() for k, v in out.items()}
    return rec, {k: ~_bits_differ(rec[k], fill[k]) for k in ARRAYS}


def _dirty(qp, b):
    """What runs on the handle between two launches of the batch: the other batch, cold, at 0.8 x0, and the certificates and the
    children of its records -- other nodes' LDS and registers, and, from the infeasible ones among them, NaN primal rows in the
    registers of kernels that are not solves (0 * what a register held is no number then)."""
    rec, _ = _launch(qp, b['x0'] * .8, b['dirty'])
    assert (rec['status'] == 1).any() and (rec['status'] == 0).any()
    qp.certify_batch(b['x0'] * .8, b['dirty'], dict(rec, iters=rec['iters'] & 0xFFFF, polished=(rec['iters'] >> 16) & 1, weak=(rec['iters'] >> 17) & 1))
    qp.branch_batch(b['dirty'], rec)


def _blocks(d):
    """Blocks of a dual row (include/hmpc.h)."""
    T, nub, o_u, o_lb = d['T'], d['nub'], d['o_u'], d['o_lb']
    return (('lam', 0, o_u), ('mu', o_u, o_lb), ('nu_lb', o_lb, o_lb + T * nub), ('nu_ub', o_lb + T * nub, o_lb + 2 * T * nub), ('rho/sigma', o_lb + 2 * T * nub, d['n_dual']))


def _where(mask, d=None):
    """'12 entries of rows [3, 9] (mu 10, lam 2)' for a mask over an array of records."""
    rows = np.flatnonzero(mask.reshape(len(mask), -1).any(axis=1))
    text = '%d entries of rows %s' % (int(mask.sum()), rows.tolist())
    if d is not None and mask.ndim == 2 and mask.shape[1] == d['n_dual'] and mask.any():
        text += ' (' + ', '.join('%s %d' % (n, int(mask[:, a:b].sum())) for n, a, b in _blocks(d) if mask[:, a:b].any()) + ')'
    return text


def _differences(a, b, d, what, lines):
    """Appends one line per array in which the records a and b differ in their bits; returns the number of such arrays."""
    n = 0
    for k in ARRAYS:
        bad = _bits_differ(np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k]))
        if bad.any():
            both = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
            with np.errstate(invalid='ignore'):
                gap = np.abs(both[0] - both[1])[bad]
            lines.append('%s: %s differs in %s, by at most %.3e' % (what, k, _where(bad, d if k == 'dual' else None), np.nanmax(gap) if np.isfinite(gap).any() else np.nan))
            n += 1
    return n


def _report(lines):
    print('\n'.join(lines))


def _misplaced(a, b, d, fix, verified):
    """Entries in which the records a and b may NOT differ, as text lines: anything but the bounds' multipliers of binaries a node
    fixes (nu_lb / nu_ub of the dual row) and the dual objective, of nodes whose handed set verified."""
    bad = []
    for k in ARRAYS:
        m = _bits_differ(np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k]))
        if k == 'dual':
            T, nub, o_lb = d['T'], d['nub'], d['o_lb']
            allowed = np.zeros(m.shape, bool)
            fixed = (fix >= 0) & verified[:, None]
            allowed[:, o_lb:o_lb + T * nub] = fixed
            allowed[:, o_lb + T * nub:o_lb + 2 * T * nub] = fixed
            m = m & ~allowed
        elif k == 'dual_obj':
            m = m & ~verified
        if m.any():
            bad.append('%s differs in %s' % (k, _where(m, d if k == 'dual' else None)))
    return bad


@pytest.mark.parametrize('batch', list(BATCHES))
@pytest.mark.parametrize('kernel', list(KERNELS))
def test_handed_records_are_written_repeatable_independent_of_company_and_certified(kernel, batch):
    b = _batch(batch)
    T, x0, fix, index, orc = b['T'], b['x0'], b['fix'], b['index'], b['orc']
    ctrl = _handle(kernel, T)
    qp, d = ctrl.qp, br.dims_of(ctrl.problem_data())
    handed = index >= 0
    lines, failed = ['%s, batch %s (%d nodes, %d handed):' % (kernel, batch, len(fix), int(handed.sum()))], []

    def certified(rec, ref, f, what):
        try:
            assert_certified(ctrl, x0, f, record_from_device(*(rec[k] for k in ARRAYS)), ref=ref, what=what)
        except AssertionError as exc:
            lines.append('  certificate: %s' % exc)
            failed.append('certificate: %s' % exc)

    with _env(KERNELS[kernel][1]):
        table, _ = _launch(qp, x0, b['table_fix'])                                # the parents' rows: this kernel's own cold records
        assert np.array_equal(table['status'], b['cold_status']) and np.all(table['iters'][index[handed]] & br.POLISHED_BIT)
        warm = (_to(table['primal']), _to(table['dual']), _to(index))
        runs, unwritten = [], []
        for r in range(3):
            _dirty(qp, b)                                                        # before every launch: other nodes' LDS and registers
            rec, left = _launch(qp, x0, fix, warm, which=r % 2)
            runs.append(rec)
            unwritten.append(left)
        host = qp.solve_batch(x0, fix, warm=(table['primal'], table['dual'], index))
        host = dict(host, iters=br.iters_word(host))
        # the handed nodes as a batch of their own, their parents' rows gathered; and in reversed order
        sub = np.flatnonzero(handed)
        own_rows = (_to(table['primal'][index[sub]]), _to(table['dual'][index[sub]]))
        alone, _ = _launch(qp, x0, fix[sub], own_rows + (_to(np.arange(len(sub), dtype=np.int32)),))
        back, _ = _launch(qp, x0, fix[sub[::-1]], own_rows + (_to(np.arange(len(sub), dtype=np.int32)[::-1].copy()),), which=1)
        children = [qp.branch_batch(fix[sub], {k: runs[r][k][sub] for k in ARRAYS}) for r in (0, 2)]

    # coverage, from the iters word
    verified = (runs[0]['iters'] & br.HANDED_BIT) != 0
    seen = _kinds(index, runs[0]['status'], runs[0]['iters'], verified)
    lines.append('  kinds of handed nodes: %s' % seen)
    assert {k for k in KINDS if seen[k]} == set(BATCHES[batch][2]), seen
    assert np.array_equal(runs[0]['status'], b['ref']['status']) and (runs[0]['status'] <= 1).all() and not (verified & ~handed).any()
    # written
    for r, left in enumerate(unwritten):
        for k in ARRAYS:
            if left[k].any():
                failed.append('unwritten: run %d, %s: %s' % (r, k, _where(left[k], d if k == 'dual' else None)))
    lines.append('  unwritten: %s' % ('; '.join(failed) or 'none'))
    # repeatable, the host-pointer entry, independent of company
    diff = []
    first = {k: runs[0][k][sub] for k in ARRAYS}
    for what, one, other, f, v in (('run 2 against run 1', runs[0], runs[1], fix, verified), ('run 3 against run 1', runs[0], runs[2], fix, verified),
                                   ('host-pointer entry against run 1', runs[0], host, fix, verified),
                                   ('the handed nodes alone against run 1', first, alone, fix[sub], verified[sub]),
                                   ('the handed nodes alone, reversed, against run 1', first, {k: back[k][::-1] for k in ARRAYS}, fix[sub], verified[sub])):
        _differences(one, other, d, what, diff)
        diff += ['%s, and not among the bounds of the fixed binaries of verified hand-downs: %s' % (what, t) for t in _misplaced(one, other, d, f, v)]
    lines += ['  ' + t for t in diff] or ['  repeatable and independent of company: every array bit-equal']
    failed += diff
    # certified, every run; downstream
    for r, rec in enumerate(runs):
        certified(rec, b['ref'], fix, 'run %d' % (r + 1))
    certified(host, b['ref'], fix, 'host-pointer entry')
    ref_sub = {k: v[sub] for k, v in b['ref'].items() if isinstance(v, np.ndarray) and len(v) == len(fix)}
    certified(alone, ref_sub, fix[sub], 'the handed nodes alone')
    certified({k: back[k][::-1] for k in ARRAYS}, ref_sub, fix[sub], 'the handed nodes alone, reversed')
    assert set(children[0]) == set(children[1]) and 'child_lb' in children[0] and children[0]['n_children'] > 0
    try:
        br.compare(children[0], children[1], what='children of run 1 and of run 3')
    except AssertionError as exc:
        lines.append('  downstream: %s' % (str(exc)[:300],))
        failed.append('downstream: %s' % (str(exc)[:300],))
    lines.append('  %d failures' % len(failed))
    _report(lines)
    assert not failed, '\n'.join(failed)


def test_a_device_search_with_hand_down_is_repeatable():
    """One T = 20 device search (K = 2, width 8, hand-down on) twice from ``begin`` in one process, another batch with its
    certificates and children on the same handle before each: the same trees, the same results, to the bit."""
    from test_gpu_branch import _backend
    from warm_start_hmpc_amd.search import DeviceSearch
    ctrl, qp, d = _backend('cart_pole_t20')
    x0 = BATCHES['B'][1]
    x0s = np.array([x0, x0 * .5])
    ds = DeviceSearch(ctrl, 2, node_cap=1024, row_cap=4096)
    seen = []
    for r in range(2):
        _dirty(qp, _batch('B'))
        ds.begin(x0s)
        counts = ds.run(8, 0., True)
        trees = [ds.tree(k) for k in range(2)]
        seen.append((counts, ds.results(), [dict(t, **{k: np.asarray(t[k])[:t['n']].copy() for k in sr.TREE_ARRAYS}) for t in trees], ds.leaves_flat()))
    (c1, res1, trees1, leaves1), (c2, res2, trees2, leaves2) = seen
    assert c1 == c2 and c1[0] > 1 and np.all(res1['state'] & sr.DONE) and not np.any(res1['state'] & (sr.FAILED | sr.OVERFLOW)), (c1, c2, res1['state'])
    assert (ds.rows(0, 64)['iters'] & br.HANDED_BIT).any()                       # (records were handed down, and some verified)
    sr.compare_dicts(res1, res2, what='results')
    sr.compare_dicts(leaves1, leaves2, what='leaves')
    for k in range(2):
        sr.compare_tree(trees1[k], trees2[k], what=('tree', k))
