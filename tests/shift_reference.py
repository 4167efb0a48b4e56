"""The warm-start node shift written once more, in extended precision, and the comparison that holds a kernel to it.

``shift_reference`` restates controller.py:431-721 of the reference (retain rule, shift of identifier and multipliers, change
of the dual objective, model error, clip and reopen) on the flat rows of ``layout.dual_slices()``.  It shares no code with
``BatchedMPC.construct_warm_start`` or with csrc/hmpc_shift.hip: every product and sum of the two mapped blocks and of the
objective change is accumulated in ``np.longdouble`` (64-bit significand), so beside a float64 evaluation it is exact.

Bounds (u = 2**-53; all derived here, none measured from a kernel)

* copies and zeros: exact.
* mapped entry  m_r = sum_k M[r, k] v[k]  (n terms): any float64 evaluation, in any order, with or without fused
  multiply-adds, errs by at most  gamma_n * S_map,  S_map = sum_k |M[r, k] v[k]|,  gamma_n ~ n u  (every term passes one
  product and at most n - 1 additions).  A kernel is allowed 4 n u S_map, the numpy form is held to n u S_map.
* objective: the shifted objective is  dobj + pi  with pi a sum of ``n_outer`` terms (one per row of each block of
  controller.py:668-721, and dobj itself), each of them a product of short inner sums.  ``S_pi`` is the sum of the absolute
  values of all elementary products of the fully expanded expression, with the squares expanded as they are COMPUTED
  ((rho/2 - Qx)^2 - (Qx)^2, not rho^2/4 - rho Qx: the cancellation is part of the arithmetic).  An elementary product passes
  at most ``n_inner`` roundings inside its term (the longest inner sum, twice for a square, the roundings of the mapped
  entry it may contain) and at most ``n_outer`` additions outside, so the error of any evaluation order is at most
  gamma_{n_pi} (|dobj| + S_pi) with  n_pi = n_outer + n_inner.  The clip max(., 0) is 1-Lipschitz: the same bound holds for
  the clipped objective and for a finite lower bound.
* flags: exact, except on leaves whose reference objective before the clip lies within that bound of zero (clip and
  reopen are discontinuous there); those are counted, and capped at 1 % of the kept leaves.
"""
import numpy as np

L = np.longdouble
U = 2.0 ** -53
assert np.finfo(L).eps <= 2.0 ** -63, 'np.longdouble is no wider than float64 on this platform: the reference needs x87 extended precision'

SEGMENTS = ('lam', 'mu', 'nu_lb', 'nu_ub', 'rho', 'sigma')


def _sizes(lay):
    return lay.T, lay.nx, lay.nu, lay.nub, lay.nc, lay.ncL, lay.nq, lay.nr, lay.nqT


def n_pi_terms(lay):
    """(n_outer, n_inner) of the module docstring."""
    T, nx, nu, nub, nc, ncL, nq, nr, nqT = _sizes(lay)
    # dobj | (rho_0/2 - Qx)^2 and (Qx)^2 | the same for sigma | mu_0 . g | nu_lb, nu_ub | rho_T^2 | rho'^2 | mu_L . h_Tm1 | mu' . h | lam_1 . e0
    n_outer = 1 + 2 * nq + 2 * nr + nc + 2 * nub + nqT + nq + ncL + nc + nx
    n_inner = max(nx + nu + 3,              # mu_0[r] * (F x0 + G u0 - h)[r]
                  2 * (nx + 2) + 1,         # (rho_0[r] / 2 - (Q x0)[r])^2
                  2 * (nu + 2) + 1,         # (sigma_0[r] / 2 - (R u0)[r])^2
                  nu + 3,                   # (lo - (V u0)[i]) * nu_lb[i]
                  2 * (nqT + 1) + 2,        # (M_rho rho_T)[r]^2 / 4, the mapped entry rounded to float64 first
                  ncL + 3)                  # h[r] * (M_mu mu_L)[r], likewise
    return n_outer, n_inner


def shift_reference(ctrl, x0, u0, e0, fix, lb, dual, dobj):
    """The shift of the leaves of ONE tree (x0, u0 = (uc0, ub0) applied, e0 model error).  Every row is shifted, kept or not;
    ``keep`` says which rows a caller may look at.  Returns a dict:

    keep [n] bool; fix [n, T nub] int8; dual [n, n_dual] float64 (mapped blocks rounded once from long double);
    obj_raw [n] long double, the shifted objective before the clip; dobj, lb [n] float64 after clip / reopen; reopened [n] bool;
    S_pi [n], S_map [n, n_dual] (zero outside the mapped blocks), n_pi, n_map [n_dual] (inner length of a mapped entry);
    bound_obj [n] = n_pi u (|dobj_in| + S_pi), bound_map [n, n_dual] = n_map u S_map  -- the bounds WITHOUT the factor 4.
    """
    lay, mld = ctrl.layout, ctrl.mld
    cut = lay.dual_slices()
    T, nx, nu, nub, nc, ncL, nq, nr, nqT = _sizes(lay)
    nuc = nu - nub
    fix = np.asarray(fix, dtype=np.int8)
    dual = np.asarray(dual, dtype=np.float64)
    n = fix.shape[0]
    assert fix.shape == (n, T * nub) and dual.shape == (n, lay.n_dual)
    x0, u0, e0 = (np.asarray(a, dtype=np.float64) for a in (x0, u0, e0))

    # retain rule (controller.py:566-613): what the leaf fixes at time 0 is what was applied
    applied = np.rint(u0[nuc:]).astype(np.int64)
    first = fix[:, :nub].astype(np.int64)
    keep = np.all((first < 0) | (first == applied[None, :]), axis=1)

    # identifier: drop time 0, the entering stage is free
    new_fix = np.full_like(fix, -1)
    for t in range(T - 1):
        new_fix[:, t * nub:(t + 1) * nub] = fix[:, (t + 1) * nub:(t + 2) * nub]

    # multipliers (controller.py:615-666), stage by stage
    new = np.zeros_like(dual)
    for name in ('lam', 'nu_lb', 'nu_ub', 'sigma'):
        for t in range(len(cut[name]) - 1):
            new[:, cut[name][t]] = dual[:, cut[name][t + 1]]
    for t in range(T - 2):
        new[:, cut['mu'][t]] = dual[:, cut['mu'][t + 1]]
    for t in range(T - 1):
        new[:, cut['rho'][t]] = dual[:, cut['rho'][t + 1]]
    D = dual.astype(L)
    M_mu, M_rho = np.asarray(ctrl._update['mu'], dtype=np.float64).astype(L), np.asarray(ctrl._update['rho'], dtype=np.float64).astype(L)
    assert M_mu.shape == (nc, ncL) and M_rho.shape == (nq, nqT)
    mu_L, rho_T = D[:, cut['mu'][T - 1]], D[:, cut['rho'][T]]
    mu_new, S_mu = mu_L.dot(M_mu.T), np.abs(mu_L).dot(np.abs(M_mu).T)
    rho_new, S_rho = rho_T.dot(M_rho.T), np.abs(rho_T).dot(np.abs(M_rho).T)
    new[:, cut['mu'][T - 2]] = mu_new.astype(np.float64)
    new[:, cut['rho'][T - 1]] = rho_new.astype(np.float64)
    S_map = np.zeros(dual.shape)
    S_map[:, cut['mu'][T - 2]] = S_mu.astype(np.float64)
    S_map[:, cut['rho'][T - 1]] = S_rho.astype(np.float64)
    n_map = np.zeros(lay.n_dual)
    n_map[cut['mu'][T - 2]] = ncL
    n_map[cut['rho'][T - 1]] = nqT

    # change of the dual objective (controller.py:668-721) and the model error (controller.py:541-558)
    lx, lu, le = x0.astype(L), u0.astype(L), e0.astype(L)
    ax, au = np.abs(lx), np.abs(lu)
    Q, R, F, G, V = (np.asarray(a, dtype=np.float64).astype(L) for a in (ctrl.Q, ctrl.R, mld.F, mld.G, mld.V))
    h, h_L = np.asarray(mld.h, dtype=np.float64).astype(L), np.asarray(ctrl.h_Tm1, dtype=np.float64).astype(L)
    qx, S_qx = Q.dot(lx), np.abs(Q).dot(ax)
    ru, S_ru = R.dot(lu), np.abs(R).dot(au)
    g, S_g = F.dot(lx) + G.dot(lu) - h, np.abs(F).dot(ax) + np.abs(G).dot(au) + np.abs(h)
    vu, S_vu = V.dot(lu), np.abs(V).dot(au)
    lo = np.where(first >= 0, first, 0).astype(L)
    hi = np.where(first >= 0, first, 1).astype(L)
    rho_0, sig_0, mu_0 = D[:, cut['rho'][0]], D[:, cut['sigma'][0]], D[:, cut['mu'][0]]
    nlb_0, nub_0, lam_1 = D[:, cut['nu_lb'][0]], D[:, cut['nu_ub'][0]], D[:, cut['lam'][1]]
    half, quarter = L(0.5), L(0.25)
    pi = np.sum((half * rho_0 - qx) ** 2 - qx ** 2, axis=1) + np.sum((half * sig_0 - ru) ** 2 - ru ** 2, axis=1)
    S = np.sum((half * np.abs(rho_0) + S_qx) ** 2 + S_qx ** 2, axis=1) + np.sum((half * np.abs(sig_0) + S_ru) ** 2 + S_ru ** 2, axis=1)
    pi = pi - mu_0.dot(g)
    S = S + np.abs(mu_0).dot(S_g)
    pi = pi - np.sum((lo - vu) * nlb_0, axis=1) - np.sum((vu - hi) * nub_0, axis=1)
    S = S + np.sum((lo + S_vu) * np.abs(nlb_0), axis=1) + np.sum((S_vu + hi) * np.abs(nub_0), axis=1)
    pi = pi + quarter * np.sum(rho_T ** 2, axis=1) - quarter * np.sum(rho_new ** 2, axis=1)
    S = S + quarter * np.sum(rho_T ** 2, axis=1) + quarter * np.sum(S_rho ** 2, axis=1)
    pi = pi + mu_L.dot(h_L) - mu_new.dot(h)
    S = S + np.abs(mu_L).dot(np.abs(h_L)) + S_mu.dot(np.abs(h))
    pi = pi - lam_1.dot(le)
    S = S + np.abs(lam_1).dot(np.abs(le))
    dobj_in = np.asarray(dobj, dtype=np.float64)
    obj_raw = dobj_in.astype(L) + pi

    # clip, and what becomes of the bound (controller.py:541-558)
    obj = np.maximum(obj_raw, L(0)).astype(np.float64)
    lb = np.asarray(lb, dtype=np.float64)
    was_inf = np.isinf(lb)
    reopened = was_inf & (obj_raw <= 0)
    new_lb = np.where(was_inf, np.where(reopened, 0.0, lb), obj)
    n_outer, n_inner = n_pi_terms(lay)
    n_pi = n_outer + n_inner
    S_pi = S.astype(np.float64)
    with np.errstate(invalid='ignore'):
        bound_obj = n_pi * U * (np.abs(dobj_in) + S_pi)
    return dict(keep=keep, fix=new_fix, dual=new, obj_raw=obj_raw, dobj=obj, lb=new_lb, reopened=reopened,
                S_pi=S_pi, S_map=S_map, n_pi=n_pi, n_map=n_map, bound_obj=bound_obj, bound_map=n_map[None, :] * U * S_map,
                tree=dict(g=g.astype(np.float64), qx=qx.astype(np.float64), ru=ru.astype(np.float64), vu=vu.astype(np.float64)))


_PER_LEAF = ('keep', 'fix', 'dual', 'obj_raw', 'dobj', 'lb', 'reopened', 'S_pi', 'S_map', 'bound_obj', 'bound_map')


def shift_reference_many(ctrl, w):
    """``shift_reference`` tree by tree over a workload ``w`` (owner, x0, u0, e0 per tree; fix, lb, dual, dobj per leaf), put
    back in the order of the leaves."""
    B = len(w['owner'])
    out = None
    for k in range(w['x0'].shape[0]):
        idx = np.flatnonzero(w['owner'] == k)
        if idx.size == 0:
            continue
        r = shift_reference(ctrl, w['x0'][k], w['u0'][k], w['e0'][k], w['fix'][idx], w['lb'][idx], w['dual'][idx], w['dobj'][idx])
        if out is None:
            out = {name: np.zeros((B,) + r[name].shape[1:], dtype=r[name].dtype) for name in _PER_LEAF}
            out['n_pi'], out['n_map'] = r['n_pi'], r['n_map']
        for name in _PER_LEAF:
            out[name][idx] = r[name]
    return out


def numpy_form_many(ctrl, w):
    """The product's float64 numpy form (``BatchedMPC.construct_warm_start``) over a workload, scattered into B rows in the
    shape of ``HipBatchedQP.shift_batch``'s result (rows of dropped leaves are undefined)."""
    from warm_start_hmpc_amd.batched import BatchedMPC, NodeArrays
    bm = BatchedMPC(ctrl)
    assert not bm.device_shift
    nuc = ctrl.layout.nuc
    B = len(w['owner'])
    out = dict(keep=np.zeros(B, bool), reopened=np.zeros(B, bool), fix=np.zeros_like(w['fix']), lb=np.zeros(B),
               dual=np.zeros_like(w['dual']), dual_obj=np.zeros(B))
    first = w['fix'][:, :ctrl.layout.nub]
    for k in range(w['x0'].shape[0]):
        idx = np.flatnonzero(w['owner'] == k)
        if idx.size == 0:
            continue
        leaves = NodeArrays(w['fix'][idx], w['lb'][idx], w['dual'][idx], w['dobj'][idx], np.ones(idx.size, bool))
        ws = bm.construct_warm_start(leaves, w['x0'][k], w['u0'][k][:nuc], w['u0'][k][nuc:], w['e0'][k])
        # (the numpy form returns the kept leaves only, in order: the same rule, restated to find their rows)
        kept = idx[np.all((first[idx] < 0) | (first[idx] == np.rint(w['u0'][k][nuc:]).astype(np.int8)), axis=1)]
        assert len(ws) == kept.size
        out['keep'][kept] = True
        out['fix'][kept], out['lb'][kept], out['dual'][kept], out['dual_obj'][kept] = ws.fix, ws.lb, ws.dual, ws.dobj
        out['reopened'][kept] = ~ws.has_dual
    return out


def where_in_row(lay, i):
    """('mu', 7) for entry i of a dual row: segment name and stage."""
    cut = lay.dual_slices()
    for name in SEGMENTS:
        for t, s in enumerate(cut[name]):
            if s.start <= i < s.stop:
                return name, t
    raise IndexError(i)


class Comparison(object):
    """What ``compare`` found: ``failures`` (name of the quantity -> list of report lines), the worst error as a fraction of
    the bound for mapped entries and for the objective, and the leaves left out of the flag comparison."""

    def __init__(self):
        self.failures = {}
        self.worst_map = self.worst_obj = 0.0
        self.excluded = self.kept = 0

    def fail(self, name, line):
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
            out.append('%s: %d mismatches' % (name, len(lines)))
            out += ['    ' + l for l in lines[:limit]]
        return '\n'.join(out)

    def figures(self):
        return 'worst error / bound: mapped %.3g, objective %.3g; %d of %d kept leaves left out of the flag comparison' % (
            self.worst_map, self.worst_obj, self.excluded, self.kept)


def compare(ctrl, ref, got, factor=4.0, stride=None, exclusion_cap=0.01, limit=6):
    """Holds a shift result ``got`` (keep, reopened, fix, lb, dual, dual_obj: B rows as ``shift_batch`` returns them) to
    ``ref`` (``shift_reference_many``).  ``factor`` multiplies the derived bounds: 4 for a kernel, 1 for the numpy form.
    ``stride``: leaves one trip of the kernel's persistent loop covers (grid x waves), to report the trip of a failing leaf."""
    lay = ctrl.layout
    cut = lay.dual_slices()
    T = lay.T
    c = Comparison()

    def leaf(b):
        return 'leaf %d (trip %s)' % (b, 'n/a' if not stride else b // stride)

    for b in np.flatnonzero(ref['keep'] != got['keep'])[:limit]:
        c.fail('keep', '%s: reference %s, got %s' % (leaf(b), ref['keep'][b], got['keep'][b]))
    kept = np.flatnonzero(ref['keep'] & got['keep'])
    c.kept = kept.size
    if kept.size == 0:
        return c
    # identifier: exact
    bad = np.argwhere(ref['fix'][kept] != got['fix'][kept])
    for j, i in bad[:limit]:
        c.fail('fix', '%s identifier entry %d (stage %d, binary %d): reference %d, got %d'
               % (leaf(kept[j]), i, i // lay.nub, i % lay.nub, ref['fix'][kept[j], i], got['fix'][kept[j], i]))
    if len(bad) > limit:
        c.failures['fix'] += [''] * (len(bad) - limit)
    # multipliers: copies and zeros exact, the two mapped blocks to their bound
    mapped = np.zeros(lay.n_dual, bool)
    mapped[cut['mu'][T - 2]] = True
    mapped[cut['rho'][T - 1]] = True
    zero = np.zeros(lay.n_dual, bool)
    for name in SEGMENTS:
        zero[cut[name][-1]] = True
    rd, gd = ref['dual'][kept], got['dual'][kept]
    with np.errstate(invalid='ignore'):
        differ = ~((rd == gd) | (np.isnan(rd) & np.isnan(gd)))
    for cols, what in ((~mapped & ~zero, 'copy'), (zero, 'zero padding')):
        bad = np.argwhere(differ & cols[None, :])
        for j, i in bad[:limit]:
            name, t = where_in_row(lay, i)
            c.fail(what, '%s entry %d (%s, stage %d, offset %d): reference %r, got %r'
                   % (leaf(kept[j]), i, name, t, i - cut[name][t].start, rd[j, i], gd[j, i]))
        if len(bad) > limit:
            c.failures[what] += [''] * (len(bad) - limit)
    for name, t in (('mu', T - 2), ('rho', T - 1)):
        s = cut[name][t]
        err = np.abs(gd[:, s] - rd[:, s])
        bound = factor * ref['bound_map'][kept][:, s]
        with np.errstate(divide='ignore', invalid='ignore'):
            frac = np.where(err == 0, 0.0, err / bound)
        frac[np.isnan(frac)] = np.inf                      # (a NaN from the kernel is an error of any size)
        if frac.size:
            c.worst_map = max(c.worst_map, float(np.max(frac)))
        bad = np.argwhere(~(err <= bound))
        for j, r in bad[:limit]:
            c.fail('mapped ' + name, '%s entry %d (%s, stage %d, row %d): reference %r, got %r, error %.3g, bound %.3g'
                   % (leaf(kept[j]), s.start + r, name, t, r, rd[j, s.start + r], gd[j, s.start + r], err[j, r], bound[j, r]))
        if len(bad) > limit:
            c.failures['mapped ' + name] += [''] * (len(bad) - limit)
    # objective and bounds
    raw = ref['obj_raw'][kept]
    fin = np.isfinite(raw)                                 # (a weak ray carries -inf: it shifts to exactly zero)
    bound = factor * ref['bound_obj'][kept]
    for what, r, g in (('objective', ref['dobj'][kept], got['dual_obj'][kept]), ('lb', ref['lb'][kept], got['lb'][kept])):
        both = np.isfinite(r) & np.isfinite(g) & fin
        err = np.where(both, np.abs(np.where(both, g, 0.) - np.where(both, r, 0.)), 0.)
        with np.errstate(divide='ignore', invalid='ignore'):
            frac = np.where(err == 0, 0.0, err / bound)
        if what == 'objective' and frac.size:
            c.worst_obj = float(np.max(frac))
        wrong = both & ~(err <= bound)
        wrong |= np.isnan(g)
        if what == 'objective':
            wrong |= ~np.isfinite(g) | (~fin & (g != r))
        for j in np.flatnonzero(wrong)[:limit]:
            c.fail(what, '%s: reference %r, got %r, bound %.3g (|dobj| + S_pi = %.3g, n_pi = %d)'
                   % (leaf(kept[j]), r[j], g[j], bound[j], ref['bound_obj'][kept[j]] / (ref['n_pi'] * U), ref['n_pi']))
        if wrong.sum() > limit:
            c.failures[what] += [''] * int(wrong.sum() - limit)
    # flags: exact away from the discontinuity of clip and reopen
    near = fin & (np.abs(raw) <= bound)
    c.excluded = int(near.sum())
    if c.excluded > exclusion_cap * kept.size:
        c.fail('exclusions', '%d of %d kept leaves lie within their bound of zero (cap %g)' % (c.excluded, kept.size, exclusion_cap))
    for what, r, g in (('reopened', ref['reopened'][kept], got['reopened'][kept]),
                       ('isinf(lb)', np.isinf(ref['lb'][kept]), np.isinf(got['lb'][kept]))):
        wrong = (r != g) & ~near
        for j in np.flatnonzero(wrong)[:limit]:
            c.fail(what, '%s: reference %s, got %s (objective before the clip %r)' % (leaf(kept[j]), r[j], g[j], float(raw[j])))
        if wrong.sum() > limit:
            c.failures[what] += [''] * int(wrong.sum() - limit)
    return c


def dual_objective_property(ctrl, w, ref, got=None, tol=1e-6):
    """For rows that are real multipliers: the shifted objective before the clip is the Lagrangian dual
    (kkt_checks.dual_objective) of the shifted multipliers, under the shifted identifier, at x1 = A x0 + B u0 + e0.  Holds the
    reference to it, and ``got`` (a kernel's result: its own shifted row and identifier, its clipped objective) if given.
    Returns (failures as report lines, worst |difference| / (1 + |value|))."""
    from kkt_checks import dual_objective
    from warm_start_hmpc_amd.subproblem_solution import DualSolution
    lay, mld = ctrl.layout, ctrl.mld
    lines, worst = [], 0.0
    x1 = w['x0'].dot(mld.A.T) + w['u0'].dot(mld.B.T) + w['e0']

    def ident(row):
        return {(q // lay.nub, q % lay.nub): float(v) for q, v in enumerate(row) if v >= 0}
    for b in np.flatnonzero(ref['keep']):
        if not np.isfinite(ref['obj_raw'][b]):
            continue
        k = w['owner'][b]
        val = dual_objective(ctrl, DualSolution.from_row(lay, 0., ref['dual'][b]).variables, ident(ref['fix'][b]), x1[k])
        d = abs(float(ref['obj_raw'][b]) - val) / (1 + abs(val))
        worst = max(worst, d)
        if not d <= tol:
            lines.append('leaf %d: reference objective %r, dual objective of its shifted row %r' % (b, float(ref['obj_raw'][b]), val))
        if got is not None and got['keep'][b]:
            val = dual_objective(ctrl, DualSolution.from_row(lay, 0., got['dual'][b]).variables, ident(got['fix'][b]), x1[k])
            d = abs(got['dual_obj'][b] - max(val, 0.)) / (1 + abs(val))
            worst = max(worst, d)
            if not d <= tol:
                lines.append('leaf %d: shifted objective %r, dual objective of the shifted row %r' % (b, got['dual_obj'][b], val))
    return lines, worst


# ---- dispatch of hmpc_launch_shift (csrc/hmpc_shift.hip), from the layout sizes ---------------------------------------------
SHIFT_WAVES = 4


def shift_lds_doubles(lay, staged):
    T, nx, nu, nub, nc, ncL, nq, nr, nqT = _sizes(lay)
    d = SHIFT_WAVES * (ncL + nqT + nx + nu) + nq * nx + nr * nu + nub * nu + nq * nqT
    if staged:
        d += ncL * nc + nc * (nx + nu + 1) + ncL
    return d


def shift_row_waves(lay):
    T, nx, nu, nub, nc, ncL, nq, nr, nqT = _sizes(lay)
    fixed = (ncL + 1) // 2 * 2 * nc + nc + nq * nqT + ncL
    fixed = (fixed + 1) // 2 * 2 + (lay.n_dual + 3) // 4 * 2
    per = (lay.n_dual + 127) // 128 * 128 + 1 + nc + nq
    per = (per + 1) // 2 * 2
    room = 160 * 1024 // 8
    return min(16, (room - fixed) // per) if fixed < room else 0


def shift_dispatch(lay, cus, B, rows=True):
    """(kernel, waves per workgroup, grid) of a shift of B leaves: 'row', 'staged' or 'unstaged'."""
    waves = shift_row_waves(lay)
    if rows and waves >= 4:
        return 'row', waves, min(cus, -(-B // waves))
    staged = shift_lds_doubles(lay, True) * 8 <= 64 * 1024
    lds = shift_lds_doubles(lay, staged) * 8
    per_cu = min(8, 160 * 1024 // lds)
    return ('staged' if staged else 'unstaged'), SHIFT_WAVES, min(cus * per_cu, -(-B // SHIFT_WAVES))


# ---- workloads: one builder each, used by the CPU and the GPU half of tests/test_shift.py -----------------------------------
import functools

from helpers import make_controller, load_fixture, lp_for, long_head_parts, random_mld, random_prefix_frontier, dive_leaf, _NoBackend

ORACLE_THREADS = 8
CART_POLE_X0 = np.array([0., 0., 1., 0.])


def _oracle_controller(mld, T, objective, terminal):
    from warm_start_hmpc_amd.controller import HybridModelPredictiveController
    from oracle.oracle_qp import OracleBatchedQP
    ctrl = HybridModelPredictiveController(mld, T, objective, terminal, backend=_NoBackend(), lp=lp_for('oracle'))
    ctrl.qp = OracleBatchedQP(ctrl.problem_data(), threads=ORACLE_THREADS)
    return ctrl


def long_head_controller():
    """helpers.long_head_parts behind the oracle: ncL = 232, more than the 192 rows one batch of the register kernel's head holds."""
    mld, T, objective, terminal = long_head_parts()
    return _oracle_controller(mld, T, objective, terminal)


@functools.lru_cache(maxsize=None)
def controller(spec):
    """spec: (nx, nuc, nub, seed, T) of helpers.random_mld, (fixture, T) or 'long_head'.  CPU oracle behind it (rows are solved
    there in both halves), multiplier map from the LP oracle.  Returns (controller, a nominal initial state)."""
    if spec == 'long_head':
        return long_head_controller(), CART_POLE_X0
    if isinstance(spec[0], str):
        return make_controller(spec[0], T=spec[1], backend='oracle', threads=ORACLE_THREADS), CART_POLE_X0
    nx, nuc, nub, seed, T = spec
    mld, objective, x0 = random_mld(nx=nx, nuc=nuc, nub=nub, seed=seed)
    return _oracle_controller(mld, T, objective, None), x0


def _binary_leaf(ctrl, spec, x0):
    """A binary-feasible leaf from x0: the optimum of a branch and bound on the cart-poles, a dive on the random MLDs."""
    T, nub = ctrl.T, ctrl.mld.nub
    if isinstance(spec[0], str) or spec == 'long_head':
        sol = ctrl.feedforward(x0, printing_period=None, frontier_width=8)[0]
        assert sol is not None
        return np.rint(np.concatenate(sol.variables['ub'])).astype(np.int8)
    return dive_leaf(ctrl.qp, ctrl.mld, x0, T)


# (the size of e0 is what reopens infeasible leaves: at 0.02 the (8, 3, 4) system reopened 1 of 78 kept infeasible leaves, at 0.1
# nine; every workload here produces leaves of all five classes)
REAL = {   # spec -> (scales of the nominal x0 per tree, size of e0, p_one of the random prefixes, dives per tree)
    (8, 3, 4, 2, 10): ((1.0, 0.7, -0.8), 0.1, 0.3, 96),
    (20, 6, 8, 0, 30): ((1.0, 0.8, -0.9), 0.1, 0.3, 96),
    (6, 2, 3, 3, 12): ((1.0, 0.6, -0.9), 0.1, 0.3, 96),
    ('cart_pole_with_walls', 20): ((1.0, 0.8, 0.9), 0.01, 0.1, 96),
    ('cart_pole_one_wall', 40): ((0.5, 0.3, 0.4), 0.01, 0.1, 96),
}


@functools.lru_cache(maxsize=None)
def real_workload(spec):
    """Rows that are real multipliers: per tree (its own x0, u0, e0) a frontier of random prefixes and of prefixes of a binary
    leaf, every other one with one binary flipped, solved on the oracle; optimal records carry their objective as bound,
    infeasible ones +inf and their Farkas ray.  u0 is the first-stage input of the tree's deepest feasible record, so that the
    prefixes of the leaf survive the retain rule; the leaves of all trees are interleaved (the owner array is not sorted)."""
    ctrl, x_nom = controller(spec)
    scales, e_size, p_one, dives = REAL[spec]
    lay = ctrl.layout
    T, nub, nx, nu = lay.T, lay.nub, lay.nx, lay.nu
    x_max = load_fixture(spec[0])['x_max'] if isinstance(spec[0], str) else np.ones(nx)
    rng = np.random.default_rng(17)
    parts = dict(owner=[], fix=[], lb=[], dual=[], dobj=[])
    x0s, u0s, e0s = [], [], []
    for k, scale in enumerate(scales):
        x0 = x_nom * scale
        leaf = _binary_leaf(ctrl, spec, x0)
        fix = np.concatenate((random_prefix_frontier(T, nub, 64, p_one=p_one, seed0=1000 + 100 * k), np.full((dives, T * nub), -1, np.int8)))
        for j in range(0, 64, 2):           # every other random prefix agrees with the leaf at time 0: infeasible leaves that are kept
            fix[j, :nub] = np.where(fix[j, :nub] >= 0, leaf[:nub], -1)
        for j in range(64, 64 + dives):
            d = int(rng.integers(1, T * nub + 1))
            fix[j, :d] = leaf[:d]
            if j % 2 == 0:
                q = int(rng.integers(0, d))
                fix[j, q] = 1 - fix[j, q]
        res = ctrl.qp.solve_batch(x0, fix)
        ok = np.flatnonzero(res['status'] <= 1)
        feas = np.flatnonzero(res['status'] == 0)
        deepest = feas[np.argmax((fix[feas] >= 0).sum(axis=1))]
        x0s.append(x0)
        u0s.append(res['primal'][deepest][(T + 1) * nx:(T + 1) * nx + nu].copy())
        e0s.append(e_size * rng.standard_normal(nx) * x_max)
        parts['owner'].append(np.full(ok.size, k, np.int32))
        parts['fix'].append(fix[ok])
        parts['lb'].append(np.where(res['status'][ok] == 0, res['obj'][ok], np.inf))
        parts['dual'].append(res['dual'][ok])
        parts['dobj'].append(np.where(res['weak'][ok] > 0, -np.inf, res['dual_obj'][ok]))
    w = {name: np.concatenate(v) for name, v in parts.items()}
    order = rng.permutation(len(w['owner']))
    w = {name: np.ascontiguousarray(v[order]) for name, v in w.items()}
    w.update(x0=np.array(x0s), u0=np.array(u0s), e0=np.array(e0s))
    return w


def synthetic_workload(ctrl, B, K, seed=0):
    """Random float64 rows (no multipliers of anything): identifiers that fix time-0 binaries -- most of them the applied
    ones --, applied binaries that round to one, +inf on a third of the bounds, and objectives placed around minus the
    change the shift makes, so that clip, reopen and still-infeasible all occur."""
    lay = ctrl.layout
    T, nub, nx, nu, nuc = lay.T, lay.nub, lay.nx, lay.nu, lay.nuc
    rng = np.random.default_rng(seed)
    owner = rng.integers(0, K, B).astype(np.int32)
    x0 = rng.random((K, nx))
    e0 = 1e-3 * rng.random((K, nx))
    u0 = rng.random((K, nu)) - 0.5
    applied = rng.integers(0, 2, (K, nub))
    applied[0] = 1
    u0[:, nuc:] = applied + 0.4 * (rng.random((K, nub)) - 0.5)
    fix = np.full((B, T * nub), -1, np.int8)
    depth = np.where(rng.random(B) < 0.6, rng.integers(1, T * nub + 1, B), 0)
    values = rng.integers(0, 2, (B, T * nub)).astype(np.int8)
    agree = rng.random(B) < 0.85
    values[agree, :nub] = applied[owner[agree]]
    cols = np.arange(T * nub)[None, :] < depth[:, None]
    fix[cols] = values[cols]
    dual = rng.random((B, lay.n_dual)) - 0.25
    lb = np.where(rng.random(B) < 1. / 3, np.inf, rng.random(B))
    w = dict(owner=owner, x0=x0, u0=u0, e0=e0, fix=fix, lb=lb, dual=dual, dobj=np.zeros(B))
    pi = shift_reference_many(ctrl, w)['obj_raw'].astype(np.float64)
    w['dobj'] = np.where(rng.random(B) < 0.5, -pi + rng.standard_normal(B), 10. * rng.standard_normal(B))
    return w


def class_counts(ref):
    """kept, dropped, finite bounds, reopened, still infeasible -- of a reference result."""
    k = ref['keep']
    return dict(kept=int(k.sum()), dropped=int((~k).sum()), finite=int((k & np.isfinite(ref['lb']) & ~ref['reopened']).sum()),
                reopened=int((k & ref['reopened']).sum()), infeasible=int((k & np.isinf(ref['lb'])).sum()))
