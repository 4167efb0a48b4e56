"""What a batch of QP records owes the solver options it was computed with (``hmpc_options`` of include/hmpc.h: tol, tol_inf,
max_iter, lazy_terminal, refine, polish, polish_tol) -- as plain functions of record dicts in the form ``solve_batch`` returns them,
of the oracle or of the HIP backend alike.  No GPU and no pytest in here: every function raises an AssertionError that begins
with its own name, so that tests/test_solver_options.py can hand each one a planted defect and ask that THIS check refuses it.

    decisions_agree   an option never moves a decision: OPTIMAL / INFEASIBLE as the tight solve has it
    bracketed         weak duality perturbed by the record's own residuals brackets the tight optimum -- no second solver
    certified_at      certificates.assert_certified with the class bases that follow from the options
    truncated         a capped solve is the uncapped solve cut off at the cap, bit for bit
    capped_iters      max_iter is a cap per pass; what an undecided record may carry
    option_is_felt    ratio tests that a kernel which ignores an option cannot pass
"""
import numpy as np

from kkt_checks import dual_residuals, primal_residuals, dual_objective, primal_objective
from certificates import assert_certified, identifier_of, BASE, CLASSES, new_margins
from warm_start_hmpc_amd.subproblem_solution import PrimalSolution, DualSolution

DEFAULTS = dict(tol=1e-8, tol_inf=1e-6, max_iter=100, lazy_terminal=1, refine=1, polish=1, polish_tol=1e-4)
TIGHT = dict(tol=1e-10, polish_tol=1e-8)                              # the solve every decision and every bracket is held against
RECORD = ('status', 'iters', 'obj', 'dual_obj', 'primal', 'dual')     # a record, bit for bit; the flag words below go with it
FLAGS = ('polished', 'weak', 'uncertified', 'handed', 'second')


def effective(options):
    """The options a solve runs with, as hmpc_create maps the struct it is given (build_host_problem): tol, tol_inf, max_iter and
    polish_tol <= 0 are the defaults; the three switches are taken as they stand (0 is 'off', not 'default')."""
    out = dict(DEFAULTS)
    for k, v in options.items():
        if k not in DEFAULTS:
            raise KeyError(k)
        if k in ('tol', 'tol_inf', 'max_iter', 'polish_tol'):
            out[k] = type(DEFAULTS[k])(v) if v > 0 else DEFAULTS[k]
        else:
            out[k] = int(v)
    return out


def passes_of(ctrl, options):
    """Solves per node at most: two where the terminal set is tried lazily (first without its rows), one otherwise."""
    return 2 if (ctrl.layout.ncL > ctrl.layout.nc and effective(options)['lazy_terminal']) else 1


def handed(rec):
    """The oracle marks a handed-down record by attempt 64 in ``polished``, the HIP backend by the key 'handed'."""
    if rec.get('handed') is not None:
        return np.asarray(rec['handed']) > 0
    return np.asarray(rec['polished']) == 64


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == 'f':                                             # bitwise, NaN included (a ray's primal row is NaN)
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return np.array_equal(a, b)


def same_records(a, b, rows=None, what='records'):
    """``a`` and ``b`` are the same records bit for bit (the rows ``rows`` of both)."""
    for k in RECORD + tuple(f for f in FLAGS if a.get(f) is not None and b.get(f) is not None):
        x, y = (np.asarray(a[k]), np.asarray(b[k])) if rows is None else (np.asarray(a[k])[rows], np.asarray(b[k])[rows])
        if not _same(x, y):
            bad = [int(i) for i in range(len(x)) if not _same(x[i], y[i])]
            raise AssertionError('%s: %s differs in %d records, first %d' % (what, k, len(bad), bad[0] if rows is None else int(np.arange(len(a[k]))[rows][bad[0]])))


# ---------------------------------------------------------------------------------------------------------------------------
def decisions_agree(rec, tight, ref=None, capped=False):
    """Where ``rec`` and the tight solve both decide a node (status <= 1) they decide alike.  Without a cap on the iterations
    (capped=False) nothing is left undecided, and the statuses are those of ``ref`` -- the oracle at the SAME options --
    element by element."""
    s, t = np.asarray(rec['status']), np.asarray(tight['status'])
    both = (s <= 1) & (t <= 1)
    flips = np.flatnonzero(both & (s != t))
    if flips.size:
        raise AssertionError('decisions_agree: %d decided nodes contradict the tight solve, first %d (%d against %d)' % (flips.size, flips[0], s[flips[0]], t[flips[0]]))
    if not capped:
        if np.any(s >= 2):
            raise AssertionError('decisions_agree: %d nodes undecided without a cap, first %d (status %d)' % ((s >= 2).sum(), np.flatnonzero(s >= 2)[0], s[s >= 2][0]))
        if ref is not None and not np.array_equal(s, np.asarray(ref['status'])):
            bad = np.flatnonzero(s != np.asarray(ref['status']))
            raise AssertionError('decisions_agree: %d statuses differ from the reference at the same options, first %d' % (bad.size, bad[0]))
    return int(both.sum())


# ---------------------------------------------------------------------------------------------------------------------------
def _parts(ctrl, x0, fix_row, rec, i):
    """(primal objective, dual objective, |r|_1, |z-|_1, |eps|_1, |gamma+|_1, |w|_inf, largest slack, |multipliers|_inf) of record i, all
    recomputed from its two rows in float64."""
    layout, nub = ctrl.layout, ctrl.mld.nub
    ident = identifier_of(fix_row, nub)
    dual = DualSolution.from_row(layout, 0., np.asarray(rec['dual'][i], dtype=np.float64)).variables
    primal = PrimalSolution.from_row(layout, fix_row, 0., np.asarray(rec['primal'][i], dtype=np.float64), False).variables
    r, z = dual_residuals(ctrl, dual)
    eps, slack = primal_residuals(ctrl, primal, ident, x0)
    return dict(p=primal_objective(ctrl, primal), d=dual_objective(ctrl, dual, ident, x0), r1=np.abs(r).sum(), zneg=np.maximum(0., -z).sum(),
                eps1=np.abs(eps).sum(), gam1=np.maximum(0., -slack).sum(), winf=np.abs(rec['primal'][i]).max(), smax=max(0., slack.max()),
                yinf=np.abs(rec['dual'][i]).max())


def bracket_delta(own, opt):
    """(delta below, delta above) of a record with the parts ``own`` beside an optimal pair with the parts ``opt`` (see bracketed)."""
    return own['r1'] * opt['winf'] + own['zneg'] * opt['smax'], opt['yinf'] * (own['eps1'] + own['gam1'])


def bracketed(ctrl, x0, fix, rec, tight, what=''):
    """Every OPTIMAL record brackets the optimum of its node:   dual_obj - delta <= tight.obj <= obj + delta.

    The node is  p* = min f(w) = sum |Q x_t|^2 + |R u_t|^2  s.t.  E w = e (initial state, dynamics), g(w) = C w - h <= 0 (the rows
    of [F G], the terminal set, the bounds of the binaries), with an optimal pair w*, (y*, z* >= 0).  A record holds a primal row
    w~ and multipliers (y, z, rho, sigma); recomputed from the rows (kkt_checks, float64): p = f(w~), d = -(|rho|^2 + |sigma|^2)/4
    - e'y - h'z, the stationarity residual r = Q'rho + R'sigma + E'y + C'z, the equality residual eps = E w~ - e and the
    violations gamma+ = max(0, g(w~)).

    BELOW.  f(w) >= rho'Qx - |rho|^2/4 for every rho (and so for sigma), hence for every w the Lagrangian is
    L(w, y, z) >= d + r'w.  At w*: E w* = e and g(w*) <= 0, so L(w*, y, z) = p* + z'g(w*) <= p* + sum over z_i < 0 of |z_i| slack_i(w*).
    Together  d <= p* + |r|_1 |w*|_inf + |z-|_1 max_i slack_i(w*)  =: p* + delta_below  -- weak duality, perturbed by the
    stationarity and sign residuals times the primal scales.
    ABOVE.  w~ is feasible for the node perturbed to E w = e + eps, g(w) <= gamma+, whose optimum p(eps, gamma+) <= p.  The
    perturbation function is convex and -(y*, z*) is a subgradient of it at 0:  p(eps, gamma+) >= p* - y*'eps - z*'gamma+.
    Together  p* <= p + |(y*, z*)|_inf (|eps|_1 + |gamma+|_1)  =: p + delta_above  -- the feasibility residuals times the
    multiplier scale.

    w* and (y*, z*) are taken from ``tight`` (the oracle at tol 1e-10, polish_tol 1e-8: its polished vertex).  tight.obj is not
    p* either: it lies within its own bracket, so its width (p_t - d_t and its own two deltas) is added on both sides, and
    4 n 2^-52 (1 + |p|) for the rounding of the recomputed sums over rows of n entries.  Nothing in delta is measured on the
    records under test but their own residuals.

    The bracket is held for the recomputed pair (d, p) AND for the scalars the record reports (dual_obj, obj): these are what a
    branch and bound prunes with.  Returns the largest fraction of delta that a record used (<= 1)."""
    x0, fix = np.asarray(x0, dtype=np.float64), np.asarray(fix)
    status = np.asarray(rec['status'])
    rows = np.flatnonzero(status == 0)
    missing = rows[np.asarray(tight['status'])[rows] != 0]
    if missing.size:
        raise AssertionError('bracketed: %s record %d is OPTIMAL, the tight solve says %d' % (what, missing[0], tight['status'][missing[0]]))
    used = 0.
    for i in rows:
        xi = x0 if x0.ndim == 1 else x0[i]
        own, opt = _parts(ctrl, xi, fix[i], rec, i), _parts(ctrl, xi, fix[i], tight, i)
        below, above = bracket_delta(own, opt)
        tb, ta = bracket_delta(opt, opt)
        n = len(rec['primal'][i]) + len(rec['dual'][i])
        width = abs(opt['p'] - opt['d']) + tb + ta + 4 * n * 2. ** -52 * (1. + abs(opt['p']))
        below, above, t = below + width, above + width, float(tight['obj'][i])
        for name, lo, hi in (('recomputed', own['d'], own['p']), ('reported', float(rec['dual_obj'][i]), float(rec['obj'][i]))):
            if not (lo - below <= t <= hi + above):
                raise AssertionError('bracketed: %s record %d does not bracket the tight optimum (%s): dual_obj - %.3e = %.12e, tight %.12e, obj + %.3e = %.12e'
                                     % (what, i, name, below, lo - below, t, above, hi + above))
            used = max(used, (lo - t) / below, (t - hi) / above)
    return used


# ---------------------------------------------------------------------------------------------------------------------------
def cost_curvature(ctrl):
    """Largest entry of the Hessian of the cost, 2 (Q'Q (+) R'R) and 2 Q_T'Q_T: kernel and oracle scale the cost by its inverse."""
    return float(max(np.abs(2. * M.T.dot(M)).max() for M in (ctrl.Q, ctrl.R, ctrl.Q_T)))


def bases_at(ctrl, options):
    """The class bases of certificates.assert_certified at these options (include/hmpc.h, hmpc_options and hmpc_result.iters):
    a ray is a proof to tol_inf; a polished record is a verified vertex, whatever tol (1e-8); an unpolished one follows tol above
    1e-8 (5e-6 tol / 1e-8) and stays at the suite's 5e-6 below.  Without refinement (refine = 0) an unpolished record may have left
    by the exit at the floor of the barrier parameter, which admits a gap of 100 tol ON THE SCALED COST: in the record's units
    100 tol max(1, H), H the largest entry of the cost's Hessian -- the gap alone, every other residual as before."""
    o = effective(options)
    unpolished = BASE['unpolished'] * max(1., o['tol'] / 1e-8)
    base = {'polished': BASE['polished'], 'unpolished': unpolished, 'infeasible': o['tol_inf'], 'weak': o['tol_inf']}
    if not o['refine']:
        base['unpolished'] = {None: unpolished, 'gap': max(unpolished, 100. * o['tol'] * max(1., cost_curvature(ctrl)))}
    return base


def certified_at(ctrl, x0, fix, rec, ref, options, what='', margins=None, widen=None):
    """certificates.assert_certified with the bases of bases_at(options).  ``ref`` -- the oracle's records at the same options --
    widens a bound by REF_FACTOR where its own residual is large, as everywhere in the suite; NOT the unpolished class at refine = 0,
    whose bound is the stated contract and nothing else.  ``widen``: the classes ``ref`` may widen at all, where it is NOT a solve at
    the same options (the oracle's default records beside its own at other options: the polished class alone -- a verified vertex
    depends on no tolerance --, see test_solver_options.py)."""
    o = effective(options)
    widen = tuple(c for c in (CLASSES if widen is None else widen) if o['refine'] or c != 'unpolished')
    try:
        return assert_certified(ctrl, x0, fix, rec, ref=ref, what=what, margins=margins, base=bases_at(ctrl, options), ref_classes=widen)
    except AssertionError as exc:
        raise AssertionError('certified_at: %s' % (exc,))


# ---------------------------------------------------------------------------------------------------------------------------
def truncated(u, r, cap, what=''):
    """``r`` (max_iter = cap) is ``u`` (no cap) cut off, where every node is solved in ONE pass: (1) a node that ``u`` finished within
    the cap has the same record in ``r``, bit for bit (NaN aware; status, iteration word and flags, both objectives, both rows);
    (2) a node that took ``u`` longer is undecided in ``r`` (MAXITER) or OPTIMAL after exactly ``cap`` iterations (the acceptable
    iterate the cap falls on); (3) no node is INFEASIBLE in ``r`` that is not in ``u``.  Returns the counts (below, at, above)."""
    ui, ri = np.asarray(u['iters']) & 0xFFFF, np.asarray(r['iters']) & 0xFFFF
    us, rs = np.asarray(u['status']), np.asarray(r['status'])
    within = ui <= cap
    try:
        same_records(u, r, rows=within, what='within the cap')
    except AssertionError as exc:
        raise AssertionError('truncated: %s cap %d: %s' % (what, cap, exc))
    over = ~within
    bad = np.flatnonzero(over & ~((rs == 2) | ((rs == 0) & (ri == cap))))
    if bad.size:
        raise AssertionError('truncated: %s cap %d: node %d took %d iterations uncapped and ends status %d after %d' % (what, cap, bad[0], ui[bad[0]], rs[bad[0]], ri[bad[0]]))
    bad = np.flatnonzero((rs == 1) & (us != 1))
    if bad.size:
        raise AssertionError('truncated: %s cap %d: node %d is INFEASIBLE under the cap and status %d without' % (what, cap, bad[0], us[bad[0]]))
    return int((ui < cap).sum()), int((ui == cap).sum()), int(over.sum())


def capped_iters(rec, cap, passes, what=''):
    """max_iter caps every pass: the iteration count (low 16 bits) is at most passes x cap.  An undecided record (status >= 2) carries
    none of the flags POLISHED, WEAK, UNCERTIFIED, HANDED -- each is raised on the exit that decides the node and on no other (its
    rows and objectives are the last iterate's and promise nothing: include/hmpc.h).  Returns the largest count."""
    it, s = np.asarray(rec['iters']) & 0xFFFF, np.asarray(rec['status'])
    bad = np.flatnonzero(it > passes * cap)
    if bad.size:
        raise AssertionError('capped_iters: %s record %d ran %d iterations, the cap is %d x %d' % (what, bad[0], it[bad[0]], passes, cap))
    und = s >= 2
    for name, flag in (('POLISHED', np.asarray(rec['polished']) > 0), ('WEAK', np.asarray(rec['weak']) > 0),
                       ('UNCERTIFIED', np.asarray(rec['uncertified']) > 0), ('HANDED', handed(rec))):
        bad = np.flatnonzero(und & flag)
        if bad.size:
            raise AssertionError('capped_iters: %s undecided record %d (status %d) carries %s' % (what, bad[0], s[bad[0]], name))
    bad = np.flatnonzero(s > 3)
    if bad.size:
        raise AssertionError('capped_iters: %s record %d has status %d' % (what, bad[0], s[bad[0]]))
    return int(it.max(initial=0))


# ---------------------------------------------------------------------------------------------------------------------------
def ray_stationarity(ctrl, rec):
    """Stationarity of every ray that claims to be a proof (INFEASIBLE, not WEAK), on the scale of certificates.residuals; NaN elsewhere."""
    out = np.full(len(rec['status']), np.nan)
    for i in np.flatnonzero((np.asarray(rec['status']) == 1) & (np.asarray(rec['weak']) == 0)):
        dual = DualSolution.from_row(ctrl.layout, 0., np.asarray(rec['dual'][i], dtype=np.float64)).variables
        zero, _ = dual_residuals(ctrl, dual)
        out[i] = np.max(np.abs(zero)) / (1. + max(np.max(np.abs(np.concatenate(dual[k]))) for k in ('lam', 'mu')))
    return out


def option_is_felt(ctrl, solve, what=''):
    """``solve(**options)`` returns the records of ONE batch at these options (everything else default).  Ratios between two
    settings of the same option on the same batch: a solver that ignores the option gives 1 and fails.
      tol_inf     the worst ray's stationarity at 1e-9 is at most 1e-2 of that at 1e-4 (the oracle: <= 1e-4 on the three cart-poles, two
                  decades to spare), and the infeasible nodes take no fewer iterations on average
      polish      polish = 0 leaves no record POLISHED
      polish_tol  the optimal nodes take MORE iterations on average at 1e-7 than at 1e-2 (the oracle: 11.6 against 6.0 on the cart-pole
                  with walls, N = 10) -- strictly: equal means are what a solver gives that never reads the option
    Returns the three figures."""
    loose, sharp = solve(tol_inf=1e-4), solve(tol_inf=1e-9)
    a, b = ray_stationarity(ctrl, loose), ray_stationarity(ctrl, sharp)
    if not (np.isfinite(a).sum() >= 10 and np.isfinite(b).sum() >= 10):
        raise AssertionError('option_is_felt: %s tol_inf: fewer than 10 rays to compare' % what)
    ratio = float(np.nanmax(b) / np.nanmax(a))
    if not ratio <= 1e-2:
        raise AssertionError('option_is_felt: %s tol_inf does not reach the rays: worst stationarity %.3e at 1e-9, %.3e at 1e-4' % (what, np.nanmax(b), np.nanmax(a)))
    inf = (np.asarray(loose['status']) == 1) & (np.asarray(sharp['status']) == 1)
    it_a, it_b = float((loose['iters'][inf] & 0xFFFF).mean()), float((sharp['iters'][inf] & 0xFFFF).mean())
    if not it_b >= it_a:
        raise AssertionError('option_is_felt: %s tol_inf: infeasible nodes take %.2f iterations at 1e-9, %.2f at 1e-4' % (what, it_b, it_a))
    plain = solve(polish=0)
    if np.any(np.asarray(plain['polished']) > 0) or np.any(handed(plain)):
        raise AssertionError('option_is_felt: %s polish = 0 returns %d POLISHED records' % (what, (np.asarray(plain['polished']) > 0).sum()))
    late, early = solve(polish_tol=1e-7), solve(polish_tol=1e-2)
    opt = (np.asarray(late['status']) == 0) & (np.asarray(early['status']) == 0)
    it_l, it_e = float((late['iters'][opt] & 0xFFFF).mean()), float((early['iters'][opt] & 0xFFFF).mean())
    if not (opt.sum() >= 10 and it_l > it_e):
        raise AssertionError('option_is_felt: %s polish_tol does not move the polish: optimal nodes take %.2f iterations at 1e-7, %.2f at 1e-2' % (what, it_l, it_e))
    return dict(tol_inf_ratio=ratio, inf_iters=(it_a, it_b), ptol_iters=(it_e, it_l))


# ---------------------------------------------------------------------------------------------------------------------------
def all_checks(ctrl, x0, fix, rec, ref, tight, options, what='', margins=None, widen=None):
    """The checks every case of the option matrix owes: decisions, iteration cap and flags, certificates, bracket.  Returns the
    largest fraction of the bracket's delta that a record used."""
    o = effective(options)
    decisions_agree(rec, tight, ref=ref if widen is None else None, capped=o['max_iter'] != DEFAULTS['max_iter'])
    capped_iters(rec, o['max_iter'], passes_of(ctrl, options), what=what)
    certified_at(ctrl, x0, fix, rec, ref, options, what=what, margins=margins, widen=widen)
    return bracketed(ctrl, x0, fix, rec, tight, what=what)


def worst_of(margins):
    """(records' worst, reference's worst) residual over the classes of a certificates.new_margins() that certified_at has filled."""
    values = [v for cls in CLASSES for v in margins[cls].values()]
    return (max(v[0] for v in values), max(v[1] for v in values)) if values else (0., 0.)


def options_line(table):
    """``table``: {case: (records' worst certificate residual, the oracle's, worst fraction of the bracket used)}."""
    return 'option margins of this run (case: worst certificate residual of the records / of the oracle, bracket used): ' + \
        '; '.join('%s: %.1e / %.1e, %.2g' % ((k,) + tuple(v)) for k, v in table.items())
