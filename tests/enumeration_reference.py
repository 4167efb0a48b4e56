"""The mixed-integer optimum by exhaustive enumeration: every one of the 2^(T nub) fully fixed leaves of a small problem solved in
ONE ``solve_batch`` of the CPU oracle, the minimum taken.  It shares no tree logic with any search of the package -- no bound, no
prune, no branching order, no shift -- so it holds what the searches and the restatements they are compared with
(``search_reference``, ``advance_reference``, ``rebase_reference``, ``anytime_reference``) could all get wrong together:

    result   the optimum, the incumbent's binaries, the input u0 that is applied and the predicted state x1
    bounds   every node's bound is a lower bound of ITS part of the cube (the theorem a warm start rests on), and no node
             that carries +inf has a feasible leaf below it
    cover    the nodes partition the cube
    bracket  what an anytime search says it has proved: lower <= optimum <= upper, upper the cost of a real leaf

Each checker returns a ``Report`` (``.ok``, ``.report()``, ``.figures()``) in the manner of ``shift_reference.compare``.

Margin: 1e-6 |v| + 1e-9, the loosest objective tolerance the suite already holds kernel against oracle (the ``dual_obj`` lines of
``_compare`` in tests/test_gpu_parity.py: rtol 1e-6, atol 1e-9).  Every workload's second-best leaf lies at least GAP = 2e-4
(relative: (second - best) / (1 + best)) above its best one -- ``assert_gap`` holds that per workload and state, so that no wrong
leaf passes inside the margin.  An infinite bound is checked exactly, without margin.

NOT reachable this way, by size alone: problems with more than one 64-bit word of binaries, and the cart-pole at its real horizons
(T = 10 .. 40: 2^40 .. 2^160 leaves).  The workloads here have 12 binaries (4096 leaves) and, once, 15 (32768)."""
import hashlib

import numpy as np

MARGIN_REL, MARGIN_ABS = 1e-6, 1e-9      # tests/test_gpu_parity.py::_compare, the dual_obj lines
RTOL = 1e-5                              # the suite's parity tolerance (tests/test_gpu_parity.py)
GAP = 2e-4
SCALES = (0.3, 1., 2., 6., 12.)
# name -> random MLD (nx, nuc, nub, seed, T) of helpers.random_mld, the scales of x0 it is enumerated at, and those at which
# every leaf is infeasible
MLDS = {'mld_6_2_3_t4': ((6, 2, 3, 3, 4), SCALES, (12.,)),
        'mld_4_2_1_t12': ((4, 2, 1, 42, 12), SCALES, ()),
        'mld_5_2_2_t6': ((5, 2, 2, 21, 6), SCALES, (12.,)),
        'random_mld_t5': ((6, 2, 3, 3, 5), (1.,), ())}           # 32768 leaves, once: the random_mld_t5 of the search tests
SMALL = ('mld_6_2_3_t4', 'mld_4_2_1_t12', 'mld_5_2_2_t6')       # 4096 leaves each: what loops and families run on
CART_POLES = {'cart_pole_t3': False, 'cart_pole_t3_terminal': True}      # cart-pole with walls, T = 3; value: the terminal set
CART_POLE_STATES = np.array([[0., 0., .5, 0.], [0., 0., 1., 0.]])
WORKLOADS = tuple(MLDS) + tuple(CART_POLES)
DISABLED = set()                         # names of checks switched off (the planted-defect test shows that each one is needed)


def margin(v):
    return MARGIN_REL * abs(v) + MARGIN_ABS


def controller(name, backend='oracle', threads=8):
    """The workload's controller.  backend: 'oracle' (a CPU oracle of its own), or an object that becomes ``ctrl.qp`` (a
    placeholder, for a caller that binds the HIP backend itself)."""
    from helpers import make_controller, random_mld
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from oracle.oracle_qp import OracleBatchedQP
    placeholder = type('Unbound', (object,), {})()
    if name in CART_POLES:
        ctrl = make_controller('cart_pole_with_walls', T=3, terminal=CART_POLES[name], backend=placeholder)
    else:
        nx, nuc, nub, seed, T = MLDS[name][0]
        mld, objective, _ = random_mld(nx=nx, nuc=nuc, nub=nub, seed=seed)
        ctrl = HybridModelPredictiveController(mld, T, objective, None, backend=placeholder)
    ctrl.qp = OracleBatchedQP(ctrl.problem_data(), threads=threads) if isinstance(backend, str) and backend == 'oracle' else backend
    return ctrl


def states(name, infeasible=None):
    """The states a workload is enumerated at, (n, nx).  infeasible: None (all), False (those with a solution expected), True."""
    if name in CART_POLES:
        return CART_POLE_STATES.copy()
    from helpers import random_mld
    nx, nuc, nub, seed, T = MLDS[name][0]
    x0 = random_mld(nx=nx, nuc=nuc, nub=nub, seed=seed)[2]
    scales = [s for s in MLDS[name][1] if infeasible is None or (s in MLDS[name][2]) == infeasible]
    return np.array([x0 * s for s in scales])


def all_leaves(nfix):
    """int8 (2^nfix, nfix): row i fixes binary k to bit k of i."""
    assert 0 < nfix < 64
    return ((np.arange(2 ** nfix, dtype=np.int64)[:, None] >> np.arange(nfix)) & 1).astype(np.int8)


def leaf_index(binaries):
    b = np.rint(np.asarray(binaries, dtype=np.float64).reshape(-1)).astype(np.int64)
    assert np.all((b == 0) | (b == 1)), b
    return int((b << np.arange(b.size)).sum())


def members(fix, nfix):
    """bool (2^nfix,): the leaves below the node ``fix`` (-1 free / 0 / 1; any pattern, not only prefixes)."""
    fix = np.asarray(fix).reshape(-1)
    assert fix.size == nfix
    fixed = np.flatnonzero(fix >= 0)
    mask = int(sum(1 << int(k) for k in fixed))
    value = int(sum(1 << int(k) for k in fixed if fix[k] == 1))
    return (np.arange(2 ** nfix, dtype=np.int64) & mask) == value


class Truth(object):
    """obj (2^nfix,): every leaf's objective, +inf where the leaf is infeasible; primal: every leaf's primal row (NaN there);
    argmin, best, second (the second-smallest objective), n_feasible; x0, nx, nu, nub, T, A, B of the problem."""

    def __init__(self, ctrl, x0, rec):
        lay = ctrl.layout
        self.x0, self.nx, self.nu, self.nub, self.T, self.nfix = np.array(x0, np.float64), lay.nx, lay.nu, lay.nub, lay.T, lay.T * lay.nub
        self.A, self.B = ctrl.mld.A, ctrl.mld.B
        self.rec = rec                   # (the oracle's records of all leaves, as solve_batch returned them)
        self.status = rec['status'].copy()
        self.obj = np.where(rec['status'] == 1, np.inf, rec['obj'])
        self.primal, self.dual = rec['primal'], rec['dual']
        self.n_feasible = int((rec['status'] == 0).sum())
        order = np.argsort(self.obj, kind='stable')
        self.argmin, self.best = int(order[0]), float(self.obj[order[0]])
        self.second = float(self.obj[order[1]])
        self.feasible = np.isfinite(self.best)

    @property
    def gap(self):
        """(second best - best) / (1 + best); inf with fewer than two feasible leaves."""
        return (self.second - self.best) / (1. + self.best) if np.isfinite(self.second) else np.inf

    def below(self, fix):
        """The smallest objective among the leaves below a node; +inf where none is feasible."""
        return float(self.obj[members(fix, self.nfix)].min())

    def row(self, leaf):
        """(x (T+1, nx), u (T, nu)) of a leaf's primal row."""
        w = self.primal[leaf]
        n = (self.T + 1) * self.nx
        return w[:n].reshape(self.T + 1, self.nx), w[n:].reshape(self.T, self.nu)


_TRUTHS = {}


def _problem_key(ctrl):
    key = getattr(ctrl, '_enumeration_key', None)
    if key is None:
        h = hashlib.sha1()
        for k, v in sorted(ctrl.problem_data().items()):
            h.update(k.encode() + np.ascontiguousarray(v, dtype=np.float64).tobytes())
        key = ctrl._enumeration_key = h.hexdigest()
    return key


def truth(ctrl, x0):
    """All leaves of the controller's problem from x0 in one ``solve_batch`` of ``ctrl.qp`` -- the CPU oracle.  Every leaf must be
    decided (status 0 or 1).  Cached per (problem, x0.tobytes())."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    key = (_problem_key(ctrl), x0.tobytes())
    if key not in _TRUTHS:
        nfix = ctrl.T * ctrl.mld.nub
        assert nfix <= 15, 'enumeration is for problems of at most 2^15 leaves'
        rec = ctrl.qp.solve_batch(x0, all_leaves(nfix))
        assert np.all((rec['status'] == 0) | (rec['status'] == 1)), np.unique(rec['status'])
        _TRUTHS[key] = Truth(ctrl, x0, rec)
    return _TRUTHS[key]


def assert_gap(t, what=''):
    """The condition the margin rests on: a second feasible leaf lies at least GAP above the best one."""
    assert not t.feasible or t.gap >= GAP, (what, 'second-best gap', t.gap, 'below', GAP)


# ---- reports -------------------------------------------------------------------------------------------------------------------------
class Report(object):
    """What a checker found: ``failures`` (name of the check -> report lines) and the figures of the run."""

    def __init__(self, kind):
        self.kind, self.failures = kind, {}
        self.nodes = self.finite = self.exact = self.proved = 0
        self.worst = -np.inf           # bounds: worst (lb - below) / (1 + |below|); result: |cost - optimum| / (1 + optimum)

    def fail(self, name, line):
        if name not in DISABLED:
            self.failures.setdefault(name, []).append(line)

    @property
    def ok(self):
        return not self.failures

    def names(self):
        return sorted(self.failures)

    def report(self, limit=6):
        out = []
        for name in self.names():
            lines = self.failures[name]
            out.append('%s: %s: %d failures' % (self.kind, name, len(lines)))
            out += ['    ' + l for l in lines[:limit]]
        return '\n'.join(out)

    def figures(self):
        if self.kind == 'bounds':
            return ('bounds: worst (lb - below) / (1 + |below|) %.3g over %d nodes: %d finite checks, %d exact-infeasible (no feasible leaf below; %d of them carry +inf)'
                    % (self.worst, self.nodes, self.finite, self.exact, self.proved))
        return '%s: worst deviation %.3g' % (self.kind, self.worst)

    def merge(self, other):
        """Adds the failures and figures of another report of the same kind (K trees of one step)."""
        for name, lines in other.failures.items():
            self.failures.setdefault(name, []).extend(lines)
        self.nodes, self.finite, self.exact, self.proved = self.nodes + other.nodes, self.finite + other.finite, self.exact + other.exact, self.proved + other.proved
        self.worst = max(self.worst, other.worst)
        return self


def hold(report, what=''):
    assert report.ok, '%s\n%s' % (what, report.report())
    return report


def hold_tree(t, fix, lb, what='', quarter=False):
    """``bounds`` and ``cover`` of a set of nodes, asserted; no node is left without a check (a finite one where a leaf below it is
    feasible, the exact one where none is) and -- quarter: at a step boundary -- at least a quarter of them get one; where the
    problem has a solution, the node above the optimum gets a finite one.  Returns the report of ``bounds``."""
    b = hold(bounds(t, fix, lb), what)
    hold(cover(fix), what)
    assert b.finite + b.exact == b.nodes == len(lb), (what, b.figures())
    assert not quarter or 4 * (b.finite + b.exact) >= b.nodes, (what, b.figures())
    assert b.finite > 0 or not t.feasible, (what, b.figures())
    return b


def _close(a, b):
    """Largest deviation of a from b relative to b's largest entry (floor 1e-2): the norm-wise measure of tests/test_gpu_parity.py."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if a.shape != b.shape or np.isnan(a).any():
        return np.inf
    return float(np.max(np.abs(a - b)) / max(1e-2, np.max(np.abs(b)))) if a.size else 0.


def result(t, cost, ub, u0=None, x1=None, tol=0., nan_without_solution=True):
    """A search's answer against the enumeration.  cost: its optimum (+inf: none); ub: the incumbent's binaries, (T nub) or
    (T, nub), or None where the path returns none (the argmin leaf is then the reference of u0 and x1); u0 (nu), x1 (nx): the
    applied input and the predicted state.  tol: the search's pruning tolerance -- with tol > 0 the search may stop at any leaf
    within tol of the optimum, so the cost must lie in [optimum, optimum + tol] and be the enumerated cost of the leaf ``ub``
    names; with tol = 0 that leaf must be the argmin."""
    r = Report('result')
    cost = float(cost)
    if not t.feasible:
        if cost != np.inf:
            r.fail('infeasible', 'no leaf is feasible, cost %r' % cost)
        if nan_without_solution and u0 is not None and not np.all(np.isnan(u0)):
            r.fail('infeasible', 'no leaf is feasible, u0 %r' % (u0,))
        r.worst = 0.
        return r
    r.worst = abs(cost - t.best) / (1. + t.best)
    if tol > 0.:
        if not (t.best - margin(t.best) <= cost <= t.best + tol + margin(t.best)):
            r.fail('cost', 'cost %.12g outside [optimum, optimum + %g], optimum %.12g' % (cost, tol, t.best))
    elif not abs(cost - t.best) <= margin(t.best):
        r.fail('cost', 'cost %.12g, optimum %.12g (second best %.12g)' % (cost, t.best, t.second))
    leaf = t.argmin
    if ub is not None:
        leaf = leaf_index(ub)
        if tol == 0. and leaf != t.argmin:
            r.fail('binaries', 'leaf %d (enumerated cost %.12g), argmin %d (%.12g)' % (leaf, t.obj[leaf], t.argmin, t.best))
        if not abs(cost - t.obj[leaf]) <= margin(t.obj[leaf]):
            r.fail('binaries', 'cost %.12g is not the enumerated cost %.12g of the leaf %d the binaries name' % (cost, t.obj[leaf], leaf))
    if not np.isfinite(t.obj[leaf]):
        return r
    x, u = t.row(leaf)
    if u0 is not None:
        dev = _close(u0, u[0])
        if not dev <= RTOL:
            r.fail('u0', 'u0 %r, the leaf\'s %r (deviation %.3g)' % (np.asarray(u0), u[0], dev))
    if x1 is not None:
        dev = _close(x1, x[1])
        if not dev <= RTOL:
            r.fail('x1', 'x1 %r, the leaf\'s %r (deviation %.3g)' % (np.asarray(x1), x[1], dev))
        if u0 is not None:
            model = t.A.dot(t.x0) + t.B.dot(np.asarray(u0, np.float64))
            dev = _close(x1, model)
            if not dev <= RTOL:
                r.fail('model', 'x1 %r is not A x0 + B u0 = %r (deviation %.3g)' % (np.asarray(x1), model, dev))
    return r


def bounds(t, fix, lb):
    """Every node (fix (n, nfix), lb (n,)) against the leaves below it.  Where a leaf below is feasible (a FINITE check): the bound
    must not exceed the minimum below by more than the margin, and a bound of +inf fails -- exactly, without margin.  Where no
    leaf below is feasible (the EXACT-INFEASIBLE check) every bound is one, +inf included.  A NaN bound fails."""
    r = Report('bounds')
    fix, lb = np.asarray(fix), np.asarray(lb, np.float64)
    assert fix.shape == (len(lb), t.nfix), (fix.shape, len(lb), t.nfix)
    for j in range(len(lb)):
        below = t.below(fix[j])
        r.nodes += 1
        if np.isnan(lb[j]):
            r.fail('nan', 'node %d carries NaN' % j)
        elif below == np.inf:                                                   # no feasible leaf below: every bound holds, +inf is the proof
            r.exact += 1
            r.proved += int(lb[j] == np.inf)
        elif lb[j] == np.inf:
            r.finite += 1
            r.fail('pruned_feasible', 'node %d carries +inf, a leaf below it is feasible at %.12g' % (j, below))
        else:
            r.finite += 1
            if lb[j] > -np.inf:
                r.worst = max(r.worst, (lb[j] - below) / (1. + abs(below)))
            if not lb[j] <= below + margin(below):
                r.fail('bound', 'node %d: bound %.12g above the minimum below it %.12g by %.3g' % (j, lb[j], below, lb[j] - below))
    return r


def cover(fix):
    """The nodes partition the cube: sum 2^free == 2^nfix, and every leaf lies below exactly one node."""
    r = Report('cover')
    fix = np.asarray(fix)
    nfix = fix.shape[1]
    volume = sum(2 ** int((f < 0).sum()) for f in fix)
    count = np.zeros(2 ** nfix, np.int64)
    for f in fix:
        count += members(f, nfix)
    r.nodes, r.worst = len(fix), float(np.abs(count - 1).max()) if count.size else 0.
    if volume != 2 ** nfix:
        r.fail('volume', 'sum 2^free = %d, the cube has %d leaves' % (volume, 2 ** nfix))
    missing, twice = np.flatnonzero(count == 0), np.flatnonzero(count > 1)
    if missing.size:
        r.fail('missing', '%d leaves below no node, first %s' % (missing.size, missing[:4]))
    if twice.size:
        r.fail('duplicated', '%d leaves below more than one node, first %s' % (twice.size, twice[:4]))
    return r


def bracket(t, lower, upper):
    """What a search says it has proved as it stands: lower <= optimum + margin; upper is +inf or the cost of an enumerated
    feasible leaf (every incumbent of the package is a fully fixed node) and not below the optimum."""
    r = Report('bracket')
    lower, upper = float(lower), float(upper)
    r.worst = (lower - t.best) / (1. + abs(t.best)) if np.isfinite(t.best) and np.isfinite(lower) else (0. if not lower > t.best else np.inf)
    if np.isnan(lower) or not lower <= (t.best + margin(t.best) if t.feasible else np.inf):
        r.fail('lower', 'lower %.12g above the optimum %.12g' % (lower, t.best))
    if np.isnan(upper):
        r.fail('upper', 'upper is NaN')
    elif upper != np.inf:
        if not t.feasible or not np.min(np.abs(t.obj[np.isfinite(t.obj)] - upper)) <= margin(upper):
            r.fail('upper_leaf', 'upper %.12g is the cost of no feasible leaf' % upper)
        if t.feasible and not upper >= t.best - margin(t.best):
            r.fail('upper', 'upper %.12g below the optimum %.12g' % (upper, t.best))
    return r
