"""The iterates of a QP solve held to the oracle's, iteration by iteration -- as plain functions of record dicts in the form
``solve_batch`` returns them, of the oracle or of the HIP backend alike.  No GPU and no pytest in here: ``mirrors`` raises an
AssertionError that begins with its own name, so that tests/test_iterate_trajectory.py can hand it planted defects and ask that
THIS check refuses them.

The observable: ``max_iter = k`` with ``polish = 0`` in one pass returns the iterate after exactly k steps -- a MAXITER record
carries the last iterate (include/hmpc.h), both write-outs divide the primal part by tau and the multipliers by tau x the cost's
scale (``output:`` of oracle/hsde_qp.c, ``write_record`` of csrc/hmpc_kernel.hip).  An interior-point method corrects itself, so a
kernel whose factorisation or sweeps lose digits ends on the same vertex and passes every end-of-solve check; its k-th iterate
does not hide them.

The yardstick is the oracle's own sensitivity to rounding: the oracle on ``ulp_twins`` of the problem -- every entry of the
data moved by 2^-52 relative, one rounding -- gives, per node and k, the ``noise`` a solver that sums in another order is
entitled to, times one factor for all kernels (FACTOR of the test module; how it was measured: DESIGN.md 3.15).

    blocks       the rows of a record split into x, u, lam, mu, nu_free, nu_fixed, rho, sig
    deviation    max |a - b| / (1 + max |b|) per node and block, and over the blocks
    ulp_twins    copies of the problem data, every float64 entry times 1 + s 2^-52, s in {-1, 0, 1}
    noise        per node, the oracle's largest deviation from any of its twins
    ratios       per node, deviation / max(noise of the node, median noise)
    mirrors      the check itself
"""
import numpy as np

UNDECIDED = 2                                                       # HMPC_MAXITER: the record carries the last iterate
BLOCKS = ('x', 'u', 'lam', 'mu', 'nu_free', 'nu_fixed', 'rho', 'sig')
EXCLUDED = {}                                                       # block: reason -- none (see blocks)
SEEDS = (11, 12, 13, 14)


def columns(layout):
    """{name: (row, column indices)} -- where the parts of a record lie in its two rows (RecordLayout, include/hmpc.h): the primal
    row is x | u, the dual row lam | mu | nu_lb | nu_ub | rho | sigma.  Every column of both rows is in exactly one entry."""
    T, nx, nu, nub = layout.T, layout.nx, layout.nu, layout.nub
    out = {'x': ('primal', np.arange((T + 1) * nx)), 'u': ('primal', (T + 1) * nx + np.arange(T * nu))}
    o = 0
    for name, width in (('lam', (T + 1) * nx), ('mu', layout.n_mu), ('nu_lb', T * nub), ('nu_ub', T * nub),
                        ('rho', T * layout.nq + layout.nqT), ('sig', T * layout.nr)):
        out[name] = ('dual', o + np.arange(width))
        o += width
    assert o == layout.n_dual and (T + 1) * nx + T * nu == layout.n_primal
    return out


def blocks(ctrl, rec, fix):
    """{block: array (nodes, width)} of a batch of records, by ``ctrl.layout``; ``fix`` (nodes, T nub; -1 free) says which binaries
    a node fixes -- the records do not.

      x, u, lam, mu, rho, sig   the columns as they stand
      nu_free                   nu_lb | nu_ub of the binaries the node leaves FREE: the multipliers of their two bound rows (0 in the
                                columns of a fixed binary)
      nu_fixed                  nu_ub - nu_lb of the binaries the node FIXES (0 in the columns of a free one).  A fixed binary has
                                ONE multiplier, of its prescribed value; both write-outs split it by sign into the two columns,
                                which is a convention of the record and not a quantity of the iterate

    No block is left out (EXCLUDED is empty).  Read for an undecided exit, both write-outs fill every column alike: lam, the [F G] and
    terminal-set rows of mu (times the row scale), the bound rows of a free binary and the split multiplier of a fixed one all
    times 1 / (tau cs); x and u are w / tau; rho = 2 Q x and sigma = 2 R u are recomputed from that x and u.  With
    ``lazy_terminal = 0`` the terminal-set rows are live in both."""
    cut = columns(ctrl.layout)
    fix = np.asarray(fix)
    out = {k: np.asarray(rec[cut[k][0]], dtype=np.float64)[:, cut[k][1]] for k in ('x', 'u', 'lam', 'mu', 'rho', 'sig')}
    lb, ub = (np.asarray(rec['dual'], dtype=np.float64)[:, cut[k][1]] for k in ('nu_lb', 'nu_ub'))
    assert fix.shape == lb.shape
    free = fix < 0
    out['nu_free'] = np.concatenate((np.where(free, lb, 0.), np.where(free, ub, 0.)), axis=1)
    out['nu_fixed'] = np.where(free, 0., ub - lb)
    return {k: out[k] for k in BLOCKS if k not in EXCLUDED}


def deviation(a, b, rows):
    """``a``, ``b``: the blocks of two batches of records; ``rows``: the nodes to compare.  Returns ({block: max |a - b| / (1 + max
    |b|) per node of ``rows``}, the maximum over the blocks per node).  An entry that is no number on one side alone counts as an
    infinite deviation."""
    rows = np.asarray(rows, dtype=np.int64)
    per = {}
    for k in b:
        x, y = a[k][rows], b[k][rows]
        if x.shape[1] == 0:
            per[k] = np.zeros(len(rows))
            continue
        d = np.abs(x - y)
        d = np.where(np.isnan(d), np.inf, d)
        per[k] = d.max(axis=1) / (1. + np.abs(y).max(axis=1))
    worst = np.max([per[k] for k in per], axis=0) if len(rows) else np.zeros(0)
    return per, worst


def ulp_twins(data, seeds=SEEDS):
    """Copies of ``problem_data()``, every float64 array multiplied entrywise by 1 + s 2^-52 with s drawn uniformly from {-1, 0, 1}
    by a generator seeded per twin: zeros stay zero, shapes and the sparsity pattern are unchanged."""
    out = []
    for seed in seeds:
        rng = np.random.default_rng(seed)
        twin = {}
        for k, v in data.items():
            if isinstance(v, np.ndarray) and v.dtype == np.float64:
                twin[k] = v * (1. + rng.integers(-1, 2, size=v.shape) * 2. ** -52)
            else:
                twin[k] = v
        out.append(twin)
    return out


def off_by(data, key, relative):
    """A copy of ``problem_data()`` with the array ``key`` scaled by 1 + relative: the planted defect of the tests."""
    out = dict(data)
    out[key] = np.asarray(data[key], dtype=np.float64) * (1. + relative)
    return out


def _undecided(records):
    return np.all([np.asarray(r['status']) == UNDECIDED for r in records], axis=0)


def noise(ctrl, fix, oracle_records, twin_records):
    """Per node the largest deviation (over the blocks) between the oracle's records and those of any of its twins at the same
    options; NaN where the node is not undecided in all of them."""
    und = _undecided([oracle_records] + list(twin_records))
    rows = np.flatnonzero(und)
    out = np.full(len(und), np.nan)
    ref = blocks(ctrl, oracle_records, fix)
    out[rows] = np.max([deviation(blocks(ctrl, t, fix), ref, rows)[1] for t in twin_records], axis=0) if len(twin_records) else 0.
    return out


def left_out_cap(nodes):
    """Nodes that may be decided on one side and undecided on another, per k: max(1, 3 %) of the batch."""
    return max(1, int(0.03 * nodes))


def left_out(records):
    """The nodes that some of ``records`` decide and others leave undecided."""
    und = [np.asarray(r['status']) == UNDECIDED for r in records]
    return np.flatnonzero(np.any(und, axis=0) & ~np.all(und, axis=0))


def ratios(ctrl, fix, rec, ref, twins):
    """(nodes compared, deviation / max(noise of the node, median noise) of each, the per-block deviations, the bound's
    denominators): the nodes undecided in ``rec``, in ``ref`` and in every twin."""
    nz = noise(ctrl, fix, ref, twins)
    rows = np.flatnonzero(_undecided([rec, ref] + list(twins)))
    per, worst = deviation(blocks(ctrl, rec, fix), blocks(ctrl, ref, fix), rows)
    if not len(rows):
        return rows, np.zeros(0), per, np.zeros(0)
    den = np.maximum(nz[rows], np.median(nz[np.isfinite(nz)]))
    if not (np.all(np.isfinite(den)) and np.all(den > 0)):
        raise AssertionError('mirrors: the noise of the reference is not finite and positive')
    return rows, worst / den, per, den


def mirrors(ctrl, fix, rec, ref, twins, k, factor, what=''):
    """``rec`` (max_iter = k, polish = 0, one pass) is the k-th iterate of ``ref`` -- the oracle at the same options --, to ``factor``
    times what the oracle itself moves on ``twins``, its records on ulp_twins of the problem:

      - the nodes undecided (status 2) in ``rec``, in ``ref`` and in every twin are compared: each ran exactly k iterations
        (``iters & 0xFFFF``), and its deviation from ``ref`` is at most factor x max(noise of the node, median noise of the batch);
      - nodes that some of them decide and others do not are left out, at most max(1, 3 %) of the batch;
      - nodes that ``rec`` and ``ref`` both decide carry equal statuses.

    ``what`` names problem and kernel family.  Returns the largest ratio deviation / max(noise, median) seen."""
    head = 'mirrors: %s k %d' % (what, k)
    s, t = np.asarray(rec['status']), np.asarray(ref['status'])
    both = np.flatnonzero((s != UNDECIDED) & (t != UNDECIDED) & (s != t))
    if both.size:
        raise AssertionError('%s node %d: decided with status %d, the reference with %d' % (head, both[0], s[both[0]], t[both[0]]))
    out = left_out([rec, ref] + list(twins))
    if out.size > left_out_cap(len(s)):
        raise AssertionError('%s: %d nodes decided on one side and undecided on another (at most %d), first %d: status %d, the reference %d'
                             % (head, out.size, left_out_cap(len(s)), out[0], s[out[0]], t[out[0]]))
    rows, ratio, per, den = ratios(ctrl, fix, rec, ref, twins)
    it = np.asarray(rec['iters'])[rows] & 0xFFFF
    bad = np.flatnonzero(it != k)
    if bad.size:
        raise AssertionError('%s node %d: undecided after %d iterations, not %d' % (head, rows[bad[0]], it[bad[0]], k))
    bad = np.flatnonzero(~(ratio <= factor))
    if bad.size:
        j = bad[int(np.argmax(np.where(np.isnan(ratio[bad]), np.inf, ratio[bad])))]
        node = int(rows[j])
        block = max(per, key=lambda name: per[name][j])
        a, b = blocks(ctrl, rec, fix)[block][node], blocks(ctrl, ref, fix)[block][node]
        d = np.abs(a - b)
        c = int(np.argmax(np.where(np.isnan(d), np.inf, d)))
        raise AssertionError('%s node %d block %s: entry %d is %.17g, the reference has %.17g -- deviation %.3e, %.3g x the reference\'s own '
                             'noise %.3e, allowed %g x (%d of %d nodes over the bound)'
                             % (head, node, block, c, a[c], b[c], per[block][j], ratio[j], den[j], factor, bad.size, len(rows)))
    return float(ratio.max(initial=0.))


def ratios_line(table):
    """``table``: {(problem, family): {k: worst ratio}}."""
    return 'trajectory ratios of this run (problem family: k ratio to the oracle\'s own 1-ulp noise ...): ' + \
        '; '.join('%s %s: %s' % (name, family, ' '.join('%d %.3g' % (k, v) for k, v in sorted(row.items()))) for (name, family), row in table.items())
