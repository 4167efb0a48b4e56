"""Every record of a batch held to its own certificate: a KKT point if the node is optimal, a Farkas ray if it is infeasible.

The multipliers of a degenerate vertex are not unique, so a ``dual`` row cannot be compared with another
solver's element by element; what any valid choice of multipliers must satisfy is the certificate.  ``residuals`` evaluates it
with the functions of ``kkt_checks.py`` (the reference's three checkers restated) in float64, from the rows as they were
written out -- nothing the solver computed for itself is trusted, ``obj`` and ``dual_obj`` included --, scaled as
``kkt_checks.check_solution`` scales them.  ``assert_certified`` sorts the records into four classes and holds each class,
residual by residual, to the project's own tolerance for it.
"""
import numpy as np

from kkt_checks import dual_residuals, primal_residuals, dual_objective, primal_objective
from warm_start_hmpc_amd.subproblem_solution import PrimalSolution, DualSolution

# residuals of an optimal record / of a ray; all of them "0 is perfect", one number per record
OPTIMAL = ('stationarity', 'sign', 'primal_equality', 'primal_inequality', 'obj', 'gap', 'dual_obj')
RAY = ('stationarity', 'sign', 'dual_obj', 'ray_quadratic', 'ray_objective', 'ray_primal')
EXACT = ('ray_quadratic', 'ray_objective', 'ray_primal')        # conditions, not measurements: they hold or they do not

# The bases are the tolerances the suite already holds such records to where it checks them at all:
BASE = {
    'polished': 1e-8,     # test_gpu_parity.test_full_size_frontier_certifies_itself (check_solution, optimal nodes)
    'unpolished': 5e-6,   # test_gpu_parity.test_streaming_kernel_baseline_config4 (records without HMPC_ITERS_POLISHED)
    'infeasible': 1e-6,   # test_full_size_frontier_certifies_itself (rays); tol_inf of kernel and oracle
    'weak': 1e-6,         # a ray flagged HMPC_ITERS_WEAK: as a ray, without the stationarity bound (it has not verified)
}
CLASSES = ('polished', 'unpolished', 'infeasible', 'weak')
REF_FACTOR = 4.           # kernel and oracle sum the same rows in different orders (64 .. 256 lanes against one thread)



EXTRA_LINES = []          # figures other test modules of a session want beside the parity margins: tests/test_gpu_parity.py writes them out with its own line


def new_margins():
    """An accumulator a caller hands to assert_certified(margins=...): per class and residual [records' worst, reference's worst]
    over the calls that PASSED with a reference -- what test_gpu_parity writes into its line of parity margins."""
    return {c: {} for c in CLASSES}


def identifier_of(fix_row, nub):
    return {(k // nub, k % nub): float(v) for k, v in enumerate(fix_row) if v >= 0}


def record_from_device(obj, dual_obj, status, iters, primal, dual):
    """A record dict as solve_batch returns it, from the arrays of the device-pointer entry (flags in ``iters``: include/hmpc.h)."""
    iters = np.asarray(iters)
    return dict(obj=np.asarray(obj), dual_obj=np.asarray(dual_obj), status=np.asarray(status), primal=np.asarray(primal),
                dual=np.asarray(dual), polished=(iters >> 16) & 1, weak=(iters >> 17) & 1)


def classify(rec):
    """Class of every record: one of CLASSES, or 'skipped' for a node that was not decided (status > 1)."""
    status, n = np.asarray(rec['status']), len(rec['status'])
    polished = np.asarray(rec['polished']) > 0 if rec.get('polished') is not None else np.zeros(n, bool)
    weak = np.asarray(rec['weak']) > 0 if rec.get('weak') is not None else np.zeros(n, bool)
    kind = np.full(n, 'skipped', dtype=object)
    kind[(status == 0) & polished] = 'polished'
    kind[(status == 0) & ~polished] = 'unpolished'
    kind[(status == 1) & ~weak] = 'infeasible'
    kind[(status == 1) & weak] = 'weak'
    return kind


def residuals(ctrl, x0, fix, rec):
    """Per record the residuals named in OPTIMAL (status 0) or RAY (status 1), NaN where a name does not apply; rows of
    status > 1 are skipped (all NaN) and marked in the boolean array under 'skipped'.  x0: one state or one per node."""
    layout, nub = ctrl.layout, ctrl.mld.nub
    x0, fix = np.asarray(x0, dtype=np.float64), np.asarray(fix)
    n = len(rec['status'])
    assert fix.shape == (n, ctrl.T * nub) and rec['dual'].shape == (n, layout.n_dual) and rec['primal'].shape == (n, layout.n_primal)
    out = {k: np.full(n, np.nan) for k in set(OPTIMAL + RAY)}
    out['skipped'] = np.asarray(rec['status']) > 1
    for i in np.flatnonzero(~out['skipped']):
        xi = x0 if x0.ndim == 1 else x0[i]
        ident = identifier_of(fix[i], nub)
        dual = DualSolution.from_row(layout, rec['dual_obj'][i], np.asarray(rec['dual'][i], dtype=np.float64)).variables
        zero, nonneg = dual_residuals(ctrl, dual)
        scale = 1. + max(np.max(np.abs(np.concatenate(dual[k]))) for k in ('lam', 'mu'))
        out['stationarity'][i] = np.max(np.abs(zero)) / scale
        out['sign'][i] = np.maximum(0., 0. - np.min(nonneg, initial=0.)) / scale
        dobj = dual_objective(ctrl, dual, ident, xi)
        out['dual_obj'][i] = abs(dobj - rec['dual_obj'][i]) / (1. + abs(dobj))
        if rec['status'][i] == 1:
            out['ray_quadratic'][i] = max(np.max(np.abs(np.concatenate(dual[k])), initial=0.) for k in ('rho', 'sigma'))
            out['ray_objective'][i] = 0. if dobj > 0. else np.inf                       # (a condition: the ray proves nothing otherwise)
            out['ray_primal'][i] = float(np.sum(~np.isnan(rec['primal'][i]))) + (0. if rec['obj'][i] == np.inf else 1.)
            continue
        primal = PrimalSolution.from_row(layout, fix[i], rec['obj'][i], np.asarray(rec['primal'][i], dtype=np.float64), False).variables
        zero, nonneg = primal_residuals(ctrl, primal, ident, xi)
        out['primal_equality'][i] = np.max(np.abs(zero))
        out['primal_inequality'][i] = np.maximum(0., 0. - np.min(nonneg))
        pobj = primal_objective(ctrl, primal)
        out['obj'][i] = abs(pobj - rec['obj'][i]) / (1. + abs(pobj))
        out['gap'][i] = abs(pobj - dobj) / (1. + abs(pobj))
    return out


def _names(cls):
    if cls in ('polished', 'unpolished'):
        return OPTIMAL
    # a WEAK ray has by definition not verified: it is exempt from the stationarity bound, and from that ONLY
    return RAY if cls == 'infeasible' else tuple(k for k in RAY if k != 'stationarity')


def worst_per_class(res, kind):
    """{class: {residual: worst over the class}} -- a NaN residual of a record that has the class counts as infinite."""
    worst = {}
    for cls in CLASSES:
        rows = kind == cls
        if rows.any():
            worst[cls] = {k: float(np.max(np.where(np.isnan(res[k][rows]), np.inf, res[k][rows]))) for k in _names(cls)}
    return worst


def _base_of(base, cls, name):
    """base[cls]: one number for every residual of the class, or {residual: number, None: every other residual}."""
    b = base[cls]
    return b.get(name, b[None]) if isinstance(b, dict) else b


def assert_certified(ctrl, x0, fix, rec, ref=None, what='', margins=None, base=BASE, ref_classes=CLASSES):
    """Every record of ``rec`` certifies itself, class by class and residual by residual, to BASE[class] -- or, where ``ref``
    (the oracle's records of the SAME workload) is given, to max(BASE[class], REF_FACTOR x the reference's worst value of that
    residual in that class).  Returns the number of records per class and of skipped ones (status > 1).  ``margins``
    (new_margins()) takes in what was measured, once everything has passed.  ``base``: other class bases than BASE -- those of
    records solved at other options than the defaults (option_checks.bases_at) --, ``ref_classes``: the classes ``ref`` may widen."""
    res, kind = residuals(ctrl, x0, fix, rec), classify(rec)
    assert np.array_equal(kind == 'skipped', res['skipped'])           # no record of status <= 1 is left out
    worst = worst_per_class(res, kind)
    ref_worst = {}
    if ref is not None:
        ref_worst = worst_per_class(residuals(ctrl, x0, fix, ref), classify(ref))
    for cls, values in worst.items():
        for name, value in values.items():
            reference = ref_worst.get(cls, {}).get(name, 0.)
            bound = 0. if name in EXACT else max(_base_of(base, cls, name), REF_FACTOR * reference if np.isfinite(reference) and cls in ref_classes else 0.)
            if not value <= bound:
                rows = np.flatnonzero(kind == cls)
                at = int(rows[np.argmax(np.where(np.isnan(res[name][rows]), np.inf, res[name][rows]))])
                raise AssertionError('%s: %s record %d fails its certificate: %s = %.3e > %.3e (reference: %.3e)'
                                     % (what or 'batch', cls, at, name, value, bound, reference))
    counts = {cls: int((kind == cls).sum()) for cls in CLASSES + ('skipped',)}
    n_inf = counts['infeasible'] + counts['weak']
    assert counts['weak'] <= max(1, n_inf // 100), (what, 'WEAK rays', counts['weak'], 'of', n_inf)
    if margins is not None and ref is not None:
        for cls, values in worst.items():
            for name, value in values.items():
                if name not in EXACT:
                    seen = margins[cls].setdefault(name, [0., 0.])
                    seen[0], seen[1] = max(seen[0], value), max(seen[1], ref_worst.get(cls, {}).get(name, 0.))
    return counts


def margins_line(margins):
    """What assert_certified has put into ``margins``: per class the worst residual of the records, the
    reference's worst value of the same residual and their ratio; and the largest ratio among the residuals whose reference
    value lies above a quarter of the base (the only place where REF_FACTOR, not the base, sets the bound)."""
    parts = []
    for cls in CLASSES:
        if not margins[cls]:
            continue
        name, (value, reference) = max(margins[cls].items(), key=lambda kv: kv[1][0])
        text = '%s: worst %s %.2e (oracle %.2e, ratio %s)' % (cls, name, value, reference, '%.2f' % (value / reference) if reference > 0 else 'n/a')
        binding = [(v / r, k) for k, (v, r) in margins[cls].items() if REF_FACTOR * r > BASE[cls]]
        if binding:
            text += ', largest ratio where the factor %g binds: %.2f (%s)' % (REF_FACTOR, max(binding)[0], max(binding)[1])
        parts.append(text)
    return 'certificate margins of this run (records vs oracle, per class): ' + ('; '.join(parts) if parts else 'none taken')
