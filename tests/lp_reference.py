"""What a record of the batched LP call must satisfy, written once in extended precision, and the problem families it is held on.

``lp(A, c, b, relax) -> obj, x, z, status, iters`` solves ``max c_k'x s.t. A x <= b_k`` (csrc/hmpc_lp.hip behind
``hmpc_lp_solve_batch``, oracle/dense_lp.c, tests/highs_lp.py).  ``residuals`` evaluates, on the caller's UNSCALED ``A, c, b``
(``relax`` applied) and with every operand cast to ``np.longdouble``, the conditions that prove a record without trusting any solver:

status 0 (optimal)     primal            max(A x - b) / (1 + |b|_inf)
                       sign              most negative multiplier (EXACT: must be 0)
                       dual              |A'z - c|_inf / (1 + |c|_inf)
                       gap               |c'x - b'z| / (1 + |c'x|)
                       obj               |obj - c'x| / (1 + sum |c_j x_j|)        (the written-out value is c'x of the written-out x)
                       complementarity   max_r z_r |b_r - a_r x| / (1 + |c'x|)
  primal + sign + dual + gap prove both vectors optimal (weak duality); complementarity says it row by row.
status 1 (empty set)   sign              as above (EXACT)
                       farkas_norm       | max_r z_r |a_r|_2  -  1 |                (the largest entry is normalised to 1 in the solver's
                                                                                    row scaling: z is written out as z~_r / |a_r|)
                       farkas_objective  0 if b'z < 0, +inf otherwise (EXACT)
                       farkas_ratio      |A'z|_inf / (-b'z)                         (<= rho, the solver's own exit rule)
                       obj_nan           0 if obj is NaN, 1 otherwise (EXACT)
status 4 (unbounded)   ray_objective     0 if c'x > 0, +inf otherwise (EXACT)
                       ray_norm          | |x|_inf - 1 |
                       ray_ratio         max(max(A x), 0) / c'x                     (<= rho)
                       obj_nan           as above (EXACT)

``rho``: hmpc_lp.hip and dense_lp.c leave with a ray at 1e-7, or at 1e-3 on the weak exit (tau <= 1e-8 kappa).  Both ratios are
invariant under the row normalisation and under the scaling of the cost (for a zero row of A, whose scale is 1, trivially), so the
written-out vectors against the unscaled data show the quantity the solver tested; the normalisation to largest entry 1 scales both
sides.  ``RHO_WEAK`` is the hard bound; ``Check.weak`` counts the records that needed more than ``RHO_STRONG``.

How small the four measured residuals of an optimal record must be is the caller's (``bounds``): tests/test_lp_certificates.py
derives it.  The two normalisations are one division per entry: ``NORM_BOUND`` = 4 roundings.  ``obj``: a sum of n products in any
order errs by at most n 2^-53 sum |c_j x_j| (the kernel: 64-lane butterfly, four waves; the oracle: serial).
"""
import functools

import numpy as np

L = np.longdouble
assert np.finfo(L).eps < 1e-18, 'np.longdouble is no wider than float64 on this platform: the reference needs x87 extended precision'
EPS = 2.0 ** -53
FLOOR = 64 * EPS           # the rounding of one 64-term wave sum of unit-scale terms (tests/certify_reference.py: the same floor)
RHO_STRONG, RHO_WEAK = 1e-7, 1e-3
NORM_BOUND = 4 * EPS

MEASURED = ('primal', 'dual', 'gap', 'complementarity')             # status 0: bounds from the caller
OPTIMAL = ('primal', 'sign', 'dual', 'gap', 'obj', 'complementarity')
EMPTY = ('sign', 'farkas_norm', 'farkas_objective', 'farkas_ratio', 'obj_nan')
UNBOUNDED = ('ray_objective', 'ray_norm', 'ray_ratio', 'obj_nan')
EXACT = ('sign', 'farkas_objective', 'ray_objective', 'obj_nan')
COLUMNS = ('primal', 'sign', 'dual', 'gap', 'obj', 'complementarity', 'farkas_norm', 'farkas_objective', 'farkas_ratio',
           'ray_objective', 'ray_norm', 'ray_ratio', 'obj_nan')
BY_STATUS = {0: OPTIMAL, 1: EMPTY, 4: UNBOUNDED}
OPTIMAL_STATUS, EMPTY_STATUS, UNBOUNDED_STATUS = 0, 1, 4


def _rows(v, B, width):
    v = np.asarray(v, dtype=np.float64)
    return np.broadcast_to(v, (B, width)) if v.ndim == 1 else v


def residuals(A, c, b, rec, relax=None):
    """{column: long double [B]} -- NaN where a column does not apply to the record's status, all NaN for status 2 and 3."""
    A64 = np.asarray(A, dtype=np.float64)
    m, n = A64.shape
    B = len(rec['status'])
    c, b = _rows(c, B, n), _rows(b, B, m)
    Al = A64.astype(L)
    norms = np.sqrt(np.sum(Al * Al, axis=1))
    norms = np.where(norms > 0, norms, L(1))
    out = {k: np.full(B, np.nan, dtype=L) for k in COLUMNS}
    one, zero = L(1), L(0)
    for k in range(B):
        st = int(rec['status'][k])
        if st not in BY_STATUS:
            continue
        ck, bk = c[k].astype(L), b[k].astype(L)
        if relax is not None and relax[k] >= 0:
            bk = bk.copy()
            bk[relax[k]] += one
        x, z = np.asarray(rec['x'][k], dtype=np.float64).astype(L), np.asarray(rec['z'][k], dtype=np.float64).astype(L)
        obj = rec['obj'][k]
        if st != UNBOUNDED_STATUS:
            out['sign'][k] = np.maximum(zero, -np.min(z))
        if st != OPTIMAL_STATUS:
            out['obj_nan'][k] = zero if np.isnan(obj) else one
        if st == OPTIMAL_STATUS:
            slack = bk - Al.dot(x)
            cx, bz = ck.dot(x), bk.dot(z)
            out['primal'][k] = np.maximum(zero, np.max(-slack)) / (one + np.max(np.abs(bk)))
            out['dual'][k] = np.max(np.abs(Al.T.dot(z) - ck)) / (one + np.max(np.abs(ck)))
            out['gap'][k] = abs(cx - bz) / (one + abs(cx))
            out['obj'][k] = abs(L(obj) - cx) / (one + np.sum(np.abs(ck * x)))
            out['complementarity'][k] = np.max(np.abs(z * slack)) / (one + abs(cx))
        elif st == EMPTY_STATUS:
            bz = bk.dot(z)
            out['farkas_norm'][k] = abs(np.max(z * norms) - one)
            out['farkas_objective'][k] = zero if bz < 0 else L(np.inf)
            out['farkas_ratio'][k] = np.max(np.abs(Al.T.dot(z))) / -bz if bz < 0 else L(np.inf)
        else:
            cx = ck.dot(x)
            out['ray_objective'][k] = zero if cx > 0 else L(np.inf)
            out['ray_norm'][k] = abs(np.max(np.abs(x)) - one)
            out['ray_ratio'][k] = np.maximum(zero, np.max(Al.dot(x))) / cx if cx > 0 else L(np.inf)
    return out


class Check(object):
    """Verdict of ``check``: ``ok``, the failing columns (``names``), one line per failing record (``report``), the worst value
    per column (``worst``) and the number of rays that needed the weak constant (``weak``)."""

    def __init__(self):
        self.failures, self.worst, self.weak = [], {}, 0

    @property
    def ok(self):
        return not self.failures

    def names(self):
        return sorted(set(name for _, name, _ in self.failures))

    def report(self):
        return '; '.join('LP %d: %s%s' % f for f in self.failures[:12]) + (' ... (%d in all)' % len(self.failures) if len(self.failures) > 12 else '')


def check(A, c, b, rec, bounds, classes=None, relax=None):
    """Holds every record of ``rec`` to the certificate of its status.  ``bounds``: {column of MEASURED: float}; ``classes``:
    the statuses the construction of the problems dictates (a record of another status fails with the name 'class')."""
    res = residuals(A, c, b, rec, relax)
    n = np.asarray(A).shape[1]
    limit = dict(bounds)
    limit.update(obj=n * EPS, farkas_norm=NORM_BOUND, ray_norm=NORM_BOUND, farkas_ratio=RHO_WEAK, ray_ratio=RHO_WEAK)
    limit.update({k: 0. for k in EXACT})
    out = Check()
    for k in range(len(rec['status'])):
        st = int(rec['status'][k])
        if classes is not None and st != int(classes[k]):
            out.failures.append((k, 'class', ' (status %d where the construction gives %d)' % (st, classes[k])))
        if st not in BY_STATUS:
            if classes is None:
                out.failures.append((k, 'class', ' (status %d: no certificate)' % st))
            continue
        for name in BY_STATUS[st]:
            v = res[name][k]
            out.worst[name] = max(out.worst.get(name, 0.), float(v))
            if not v <= limit[name]:                 # (NaN fails)
                out.failures.append((k, name, ' = %.3e > %.3e' % (float(v), limit[name])))
        for name in ('farkas_ratio', 'ray_ratio'):
            if name in BY_STATUS[st] and res[name][k] > RHO_STRONG:
                out.weak += 1
    out.residuals = res
    return out


def worst_of(res, status):
    """{column of MEASURED: worst value over the optimal records} of ``residuals``' result."""
    sel = np.asarray(status) == OPTIMAL_STATUS
    return {k: float(np.max(res[k][sel], initial=L(0))) for k in MEASURED}


# ---- launch geometry of hmpc_lp_solve_batch, restated (csrc/hmpc_lp.hip: hmpc_lp_lds_bytes and the lines before the launch) ----
LP_WAVES = 4
LDS_MAX = 160 * 1024


def lds_bytes(n, m, a_in_lds):
    return 8 * (11 * m + n * n + 9 * n + 4 * LP_WAVES + (n * m if a_in_lds else 0))


def geometry(n, m, B, cus, lds_max=LDS_MAX):
    """(a_in_lds, per_cu, grid) of a batch of B LPs with m rows (every appended row counted) and n columns."""
    assert lds_bytes(n, m, 0) <= lds_max
    a_in_lds = lds_bytes(n, m, 1) <= lds_max
    per_cu = max(1, min(4, lds_max // lds_bytes(n, m, a_in_lds)))
    return a_in_lds, per_cu, min(B, cus * per_cu)


def successions(classes, grid):
    """The ordered pairs (class of the LP a workgroup has just left, class of the one it starts) of the grid-stride loop."""
    classes = np.asarray(classes)
    return set(zip(classes[:-grid].tolist(), classes[grid:].tolist())) if grid < len(classes) else set()


def wraparound_order(classes, grid, seed=0):
    """A permutation of the batch under which some workgroup sees each of the nine ordered pairs of classes: seeds are tried in
    order until one does.  With k mod 3 classes and a grid that is a multiple of 3 the identity order gives three pairs only."""
    classes = np.asarray(classes)
    want = set((a, b) for a in BY_STATUS for b in BY_STATUS)
    for s in range(seed, seed + 64):
        perm = np.random.RandomState(s).permutation(len(classes))
        if successions(classes[perm], grid) >= want:
            return perm
    raise AssertionError('no order of %d LPs on %d workgroups shows all nine successions' % (len(classes), grid))


# ---- problem families: deterministic from a seed, one A per batch --------------------------------------------------------------
MIXED_SHAPES = ((1, 1), (1, 3), (2, 9), (5, 40), (12, 70), (34, 150), (64, 62), (64, 300), (3, 1700))    # (n, m): m rows drawn, + 2


def mixed_family(n, m, B, seed=0):
    """(A [m + 2, n], c [B, n], b [B, m + 2], classes [B]): LP k is optimal / empty / unbounded for k mod 3 = 0 / 1 / 2.

    d0 is a recession direction of every set (a_r . d0 <= 0 on the drawn rows, = 0 on the appended pair a, -a), x_in lies strictly
    inside (b = A x_in + rand + 0.1).  Optimal: c = A'w, w >= 0 on min(n + 2, m) rows -- dual feasible, hence bounded.  Empty: the
    pair's right-hand sides a.x_in - 1 and -a.x_in - 1 contradict each other (multipliers 1, 1: b'z = -2).  Unbounded:
    c <- c + (1 - c.d0) d0, so c.d0 = 1 along a direction the set never leaves."""
    rng = np.random.RandomState(1000 * n + m + 7919 * seed)
    d0 = rng.randn(n); d0 /= np.linalg.norm(d0)
    A = rng.randn(m, n)
    A[A.dot(d0) > 0] *= -1.
    a = rng.randn(n); a -= a.dot(d0) * d0
    if n == 1:
        a = np.zeros(1)                       # nothing is orthogonal to d0 in R^1 but 0: the pair reads 0 <= b
    A = np.vstack((A, a, -a))
    x_in = rng.randn(n)
    b = A.dot(x_in) + rng.rand(B, m + 2) + .1
    c = np.empty((B, n))
    classes = np.array([(OPTIMAL_STATUS, EMPTY_STATUS, UNBOUNDED_STATUS)[k % 3] for k in range(B)], dtype=np.int32)
    for k in range(B):
        w = np.zeros(m + 2)
        rows = rng.permutation(m)[:min(n + 2, m)]
        w[rows] = rng.rand(rows.size) + .1
        c[k] = A.T.dot(w)
        if classes[k] == EMPTY_STATUS:
            b[k, m], b[k, m + 1] = a.dot(x_in) - 1., -a.dot(x_in) - 1.
        elif classes[k] == UNBOUNDED_STATUS:
            c[k] += (1. - c[k].dot(d0)) * d0
    return A, c, b, classes


DEGENERATE_SIZES = (2, 5, 12)


def degenerate_family(n, B=8, seed=0):
    """(A, c [B, n], b [m], V): 3n rows through the point V, the first two of them listed twice, a box of half-width 5 around V, one
    all-zero row with b = 1.  Costs in the cone of n of the rows through V (cost 0: exactly row 0), so every LP is optimal at V with
    value c'V -- 3n + 2 rows through an n-dimensional vertex, duplicates, a zero row and a cost parallel to a row: the inputs on
    which the purification walk's tie-break (the lowest-numbered blocking row) decides."""
    rng = np.random.RandomState(50 + n + 7919 * seed)
    V = rng.randn(n)
    R = rng.randn(3 * n, n) * (.5 + rng.rand(3 * n, 1) * 2.)
    A = np.vstack((R, R[:2], np.eye(n), -np.eye(n), np.zeros((1, n))))
    b = np.concatenate((R.dot(V), R[:2].dot(V), V + 5., -V + 5., [1.]))
    c = np.empty((B, n))
    for k in range(B):
        rows = rng.permutation(3 * n)[:n]
        c[k] = R[rows].T.dot(rng.rand(n) + .1)
    c[0] = R[0]
    return A, c, b, V


@functools.lru_cache(maxsize=None)
def solved(kind, n, m, B, seed=0, threads=8):
    """One family and the oracle's records of it, solved once and shared (callers leave the arrays unchanged)."""
    from oracle.oracle_lp import lp_solve_batch
    if kind == 'mixed':
        A, c, b, classes = mixed_family(n, m, B, seed)
        extra = None
    else:
        A, c, b, extra = degenerate_family(n, B, seed)
        classes = np.zeros(B, dtype=np.int32)
    return A, c, b, classes, extra, lp_solve_batch(A, c, b, threads=threads)
