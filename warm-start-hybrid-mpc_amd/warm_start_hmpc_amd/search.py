"""K branch-and-bound searches whose trees live on the device (``hmpc_search_*``, include/hmpc_search.h).

``BatchedMPC.feedforward_many`` keeps its trees in numpy and ships every round's identifiers, bounds and multipliers across the
bus; ``FleetMPC`` keeps the multiplier rows in HBM but selects, stages and consumes on the host.  Here the trees, the record
pool and the three steps around the solve (csrc/hmpc_search.hip) stay on the device: a round reads back one word, the size of
the next launch.  Per tree the semantics are those of ``_Tree.candidates`` / ``BatchedMPC._consume`` (the reference's
``branch_and_bound.py:462-489`` with the brancher of ``controller.py:395-429``).
"""
import ctypes
from time import perf_counter

import numpy as np

from .batched import NodeArrays
from . import branch_and_bound as bb
from .qp_backend import SEARCH_RULES, SEARCH_STATES, SEARCH_STOP_STATES, _Result, _Warm

# the reference's candidate_selection functions (branch_and_bound.py) as rules of the device search
_RULE_OF_SELECTION = {bb.best_first: 'best', bb.depth_first: 'depth', bb.breadth_first: 'breadth'}


class SearchTooBig(RuntimeError):
    """A round's records do not fit the pool (``row_cap``); nothing has changed."""


class DeviceSearch(object):
    """K independent MIQP searches per call, advanced in lockstep on the controller's GPU backend.

    node_cap : nodes a tree may hold (a tree that needs more stops with the OVERFLOW state)
    row_cap  : rows of the record pool, one per solved node of a step and one per leaf of the covers (default K * node_cap)
    speculation : depth s in 0 .. 4 (``set_speculation``).  Every picked node that has to be launched rides with all its
               descendants through its next s binaries; their records wait in the pool, and a later pick of such a descendant
               costs no launch.  With ``handdown=False`` the searches are those of s = 0 bit for bit, in fewer launches; with
               hand-down on the descendants are solved cold and results agree to the solver's tolerance only.  A step then needs
               up to 2^(s+1) - 1 pool rows per launched pick instead of one: the default ``row_cap`` stays, so give a larger
               one where ``SearchTooBig`` is raised.
    rule     : 'best' (the default: smallest bound first), 'depth' (the newest candidate first), 'breadth' (the oldest first) or
               'dive' (per tree depth-first until it has an incumbent, best-first from then on) -- ``set_rule``.
    max_solves : None, or the nodes a tree may consume per step (``set_budget``).  A tree that runs out of it with candidates
               left stops with the state ``SEARCH_STOP_STATES['budget']`` (and ``SEARCH_STATES['incumbent']`` with it if it has
               one); ``bounds()`` says what it has proved, and ``advance`` takes it if it has an incumbent.
    """

    def __init__(self, controller, K, node_cap=1024, row_cap=None, speculation=0, rule='best', max_solves=None):
        qp = controller.qp
        if not hasattr(qp, 'handle') or not hasattr(qp, 'lib'):
            raise RuntimeError('DeviceSearch needs the HIP backend (the product path has no CPU fallback).')
        self.c, self.qp, self.K = controller, qp, int(K)
        self.node_cap = int(node_cap)
        self.row_cap = int(row_cap) if row_cap is not None else self.K * self.node_cap
        self.nx, self.nu, self.nfix = qp.nx, qp.nu, qp.nfix
        self.n_primal, self.n_dual = qp.n_primal, qp.n_dual
        s = ctypes.c_void_p()
        rc = qp.lib.hmpc_search_create(qp.handle, self.K, self.node_cap, self.row_cap, ctypes.byref(s))
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)('hmpc_search_create failed (%d): %s' % (rc, qp.lib.hmpc_last_error().decode()))
        self._s = s
        self.rounds, self.launched = 0, 0
        self._B = self._P = 0
        self.speculation = 0
        if speculation:
            self.set_speculation(speculation)
        self.rule, self.max_solves = 'best', None
        if rule != 'best':
            self.set_rule(rule)
        if max_solves is not None:
            self.set_budget(max_solves)

    def __del__(self):
        s = getattr(self, '_s', None)
        if s:
            self.qp.lib.hmpc_search_destroy(s)
            self._s = None

    def _check(self, rc):
        if rc == -3:
            raise SearchTooBig(self.qp.lib.hmpc_last_error().decode())
        self.qp._check(rc)

    def set_speculation(self, depth):
        """Speculation depth of the rounds to come, 0 .. 4; not while a round is staged.  Waiting records stay valid."""
        rc = self.qp.lib.hmpc_search_set_speculation(self._s, int(depth))
        if rc == -1:
            raise ValueError('hmpc_search_set_speculation failed: %s' % self.qp.lib.hmpc_last_error().decode())
        self._check(rc)
        self.speculation = int(depth)

    def set_rule(self, rule):
        """The order in which the rounds to come pick among a tree's candidates: a key of ``SEARCH_RULES`` (or its code, or one
        of the three selection functions of ``branch_and_bound.py``); not while a round is staged.  It holds until it is changed."""
        name = _RULE_OF_SELECTION.get(rule, rule) if callable(rule) else rule
        if callable(name):
            raise ValueError('no rule of the device search for the selection function %r.' % (rule,))
        if not isinstance(name, str):
            name = {v: k for k, v in SEARCH_RULES.items()}.get(name, name)
        if name not in SEARCH_RULES:
            raise ValueError('rule must be one of %s.' % ', '.join(sorted(SEARCH_RULES)))
        rc = self.qp.lib.hmpc_search_set_rule(self._s, SEARCH_RULES[name])
        if rc == -1:
            raise ValueError('hmpc_search_set_rule failed: %s' % self.qp.lib.hmpc_last_error().decode())
        self._check(rc)
        self.rule = name

    def set_budget(self, max_solves, stream=None):
        """The nodes a tree may consume per step from here on (None or negative: no budget); trees that an earlier budget had
        stopped run again, so ``set_budget(None)`` -> ``run`` finishes a cut-off search.  Not while a round is staged."""
        m = -1 if max_solves is None or max_solves < 0 else int(max_solves)
        rc = self.qp.lib.hmpc_search_set_budget(self._s, m, ctypes.c_void_p(stream))
        if rc == -1:
            raise ValueError('hmpc_search_set_budget failed: %s' % self.qp.lib.hmpc_last_error().decode())
        self._check(rc)
        self.max_solves = None if m < 0 else m

    def bounds(self, tol=0., stream=None):
        """What every tree proves as it stands: dict lower (min over its leaves' bounds and the bounds of leaves pruned on
        uncertified records: a lower bound of the MIQP's cost; +inf without leaves, -inf for a root), upper (the incumbent's
        cost, +inf without one), open (candidates left at ``tol``).  Not while a round is staged."""
        out = dict(lower=np.empty(self.K), upper=np.empty(self.K), open=np.empty(self.K, dtype=np.int32))
        rc = self.qp.lib.hmpc_search_bounds(self._s, float(tol), out['lower'].ctypes.data, out['upper'].ctypes.data, out['open'].ctypes.data,
                                            ctypes.c_void_p(stream))
        if rc == -1:
            raise ValueError('hmpc_search_bounds failed: %s' % self.qp.lib.hmpc_last_error().decode())
        self._check(rc)
        return out

    def counters(self):
        """Since ``begin``: dict rounds, launches (rounds that launched QPs), rows (nodes launched), served (picks consumed
        from waiting records)."""
        out = (ctypes.c_int64 * 4)()
        self._check(self.qp.lib.hmpc_search_counters(self._s, out))
        return dict(zip(('rounds', 'launches', 'rows', 'served'), (int(v) for v in out)))

    # ------------------------------------------------------------------
    def begin(self, x0s, warm_starts=None):
        """A step begins from the states x0s (K, nx).  warm_starts: None (every tree is its root) or a list of K ``NodeArrays``
        (None entries: the root) whose leaves become the trees, with the dual rows they carry."""
        x0s = np.ascontiguousarray(np.atleast_2d(x0s), dtype=np.float64)
        if x0s.shape != (self.K, self.nx):
            raise ValueError('x0s must have shape (%d, %d).' % (self.K, self.nx))
        if warm_starts is None:
            self._check(self.qp.lib.hmpc_search_begin(self._s, x0s.ctypes.data, None, None, None, None, None))
            return
        if len(warm_starts) != self.K:
            raise ValueError('one warm start per tree.')
        ws = [NodeArrays.root(self.nfix, self.n_dual) if w is None else w for w in warm_starts]
        count = np.array([len(w) for w in ws], dtype=np.int32)
        cat = lambda name, dtype: np.ascontiguousarray(np.concatenate([getattr(w, name) for w in ws]), dtype=dtype)
        fix, lb, dual, dobj = cat('fix', np.int8), cat('lb', np.float64), cat('dual', np.float64), cat('dobj', np.float64)
        if fix.shape != (count.sum(), self.nfix) or dual.shape != (count.sum(), self.n_dual):
            raise ValueError('warm starts have inconsistent shapes.')
        self._check(self.qp.lib.hmpc_search_begin(self._s, x0s.ctypes.data, count.ctypes.data, fix.ctypes.data, lb.ctypes.data,
                                                  dual.ctypes.data, dobj.ctypes.data))

    def select(self, frontier_width=8, tol=0., handdown=True, stream=None):
        """Stages the next round and returns its size B, the rows to solve -- the one synchronisation of a round.  The number
        of picks is in ``self._P``: the search has stopped when it is 0 (without speculation that is B == 0; with it a round
        whose picks all have waiting records has B == 0 and is still consumed).
        Raises ``SearchTooBig``, with nothing changed, when the round's records do not fit the pool."""
        B, P = ctypes.c_int32(), ctypes.c_int32()
        self._B = self._P = 0
        self._check(self.qp.lib.hmpc_search_select(self._s, int(frontier_width), float(tol), int(bool(handdown)), ctypes.byref(B),
                                                   ctypes.c_void_p(stream)))
        self._check(self.qp.lib.hmpc_search_staged(self._s, ctypes.byref(P), None))
        self._B, self._P = B.value, P.value
        return B.value

    def batch(self, device=False):
        """The staged round.  Host form: dict x0 (B, nx), fix (B, nfix), warm (B: row handed down or -1), tree, node (B), row0.
        ``device=True``: the raw device pointers instead -- dict x0, fix, warm (primal, dual, index, rows), rows (the six
        members of ``hmpc_result`` at row0 of the pool), row0 -- ready for ``hmpc_solve_batch_device``."""
        lib = self.qp.lib
        if device:
            x0, fix, warm, rows, row0 = ctypes.c_void_p(), ctypes.c_void_p(), _Warm(), _Result(), ctypes.c_int32()
            self._check(lib.hmpc_search_batch(self._s, ctypes.byref(x0), ctypes.byref(fix), ctypes.byref(warm), ctypes.byref(rows), ctypes.byref(row0)))
            return dict(x0=x0.value, fix=fix.value, warm=warm, rows=rows, row0=row0.value)
        B = self._B
        row0 = ctypes.c_int32()
        self._check(lib.hmpc_search_batch(self._s, None, None, None, None, ctypes.byref(row0)))
        out = dict(x0=np.empty((B, self.nx)), fix=np.empty((B, self.nfix), dtype=np.int8), warm=np.empty(B, dtype=np.int32),
                   tree=np.empty(B, dtype=np.int32), node=np.empty(B, dtype=np.int32))
        if B:
            self._check(lib.hmpc_search_get_batch(self._s, B, *[out[k].ctypes.data for k in ('x0', 'fix', 'warm', 'tree', 'node')]))
        out['row0'] = row0.value
        return out

    @staticmethod
    def _records(rec, B, n_primal, n_dual, empty=False):
        from .qp_backend import iters_word
        shapes = dict(obj=((B,), np.float64), dual_obj=((B,), np.float64), status=((B,), np.int32), iters=((B,), np.int32),
                      primal=((B, n_primal), np.float64), dual=((B, n_dual), np.float64))
        if empty:
            keep = {k: np.empty(*v) for k, v in shapes.items()}
        else:
            keep = {k: np.ascontiguousarray(iters_word(rec) if k == 'iters' else rec[k], dtype=shapes[k][1])
                    for k in shapes if k == 'iters' or rec.get(k) is not None}
            for k, a in keep.items():
                if a.shape != shapes[k][0]:
                    raise ValueError('record arrays have inconsistent shapes (%s).' % k)
        return keep, _Result(**{k: v.ctypes.data for k, v in keep.items()})

    def put_records(self, rec):
        """Host records (a dict as ``solve_batch`` returns it, or with the ``iters`` word of the C ABI) into the rows of the
        staged round."""
        keep, r = self._records(rec, self._B, self.n_primal, self.n_dual)
        self._check(self.qp.lib.hmpc_search_put_records(self._s, self._B, ctypes.byref(r)))

    def rows(self, first, count, rec=None):
        """Rows of the pool: read (a dict of arrays, ``iters`` the word of the C ABI) or, with ``rec``, written."""
        keep, r = self._records(rec, count, self.n_primal, self.n_dual, empty=rec is None)
        self._check(self.qp.lib.hmpc_search_rows(self._s, int(first), int(count), ctypes.byref(r), int(rec is not None)))
        return keep

    def consume(self, tol=0., stream=None):
        self._check(self.qp.lib.hmpc_search_consume(self._s, float(tol), ctypes.c_void_p(stream)))
        self._B = self._P = 0

    def run(self, frontier_width=8, tol=0., handdown=True, max_rounds=0, stream=None):
        """select -> solve -> consume until every tree has stopped.  Returns (rounds, nodes launched); ``counters()`` says how
        many of the rounds launched QPs."""
        r, n = ctypes.c_int32(), ctypes.c_int64()
        self._check(self.qp.lib.hmpc_search_run(self._s, int(frontier_width), float(tol), int(bool(handdown)), int(max_rounds),
                                                ctypes.c_void_p(stream), ctypes.byref(r), ctypes.byref(n)))
        self.rounds += r.value
        self.launched += n.value
        return r.value, n.value

    def results(self):
        """dict of per-tree arrays: cost (+inf without incumbent), u0 (K, nu), x1 (K, nx) (NaN without one), binaries (K, nfix),
        solves, leaves, state (``SEARCH_STATES``), uncertified."""
        K = self.K
        out = dict(cost=np.empty(K), u0=np.empty((K, self.nu)), x1=np.empty((K, self.nx)), binaries=np.empty((K, self.nfix), dtype=np.int8),
                   solves=np.empty(K, dtype=np.int32), leaves=np.empty(K, dtype=np.int32), state=np.empty(K, dtype=np.int32),
                   uncertified=np.empty(K, dtype=np.int32))
        self._check(self.qp.lib.hmpc_search_results(self._s, *[out[k].ctypes.data for k in ('cost', 'u0', 'x1', 'binaries', 'solves', 'leaves', 'state', 'uncertified')]))
        return out

    def leaves_flat(self):
        """The alive nodes of all trees, tree by tree in list order: dict owner, fix, lb, dual, dual_obj, has_dual."""
        lib = self.qp.lib
        n = ctypes.c_int32(0)
        rc = lib.hmpc_search_leaves(self._s, ctypes.byref(n), None, None, None, None, None, None)
        if rc not in (0, -3):
            self._check(rc)
        N = n.value
        out = dict(owner=np.empty(N, dtype=np.int32), fix=np.empty((N, self.nfix), dtype=np.int8), lb=np.empty(N), dual=np.empty((N, self.n_dual)),
                   dual_obj=np.empty(N), has_dual=np.empty(N, dtype=np.uint8))
        self._check(lib.hmpc_search_leaves(self._s, ctypes.byref(n), *[out[k].ctypes.data for k in ('owner', 'fix', 'lb', 'dual', 'dual_obj', 'has_dual')]))
        assert n.value == N
        out['has_dual'] = out['has_dual'].astype(bool)
        return out

    def leaves(self):
        """One ``NodeArrays`` per tree: its leaves with the dual rows they carry (the warm start's raw material)."""
        f = self.leaves_flat()
        out = []
        for k in range(self.K):
            m = f['owner'] == k
            out.append(NodeArrays(f['fix'][m], f['lb'][m], f['dual'][m], f['dual_obj'][m], f['has_dual'][m]))
        return out

    def advance(self, errors=None, x0_next=None, stats=True, stream=None):
        """The step that ended becomes the cover of the next one without leaving the device (``hmpc_search_advance``): retain ->
        shift -> adopt for all K trees, then the state of a fresh ``begin``.  errors (K, nx): the model errors of the step (None:
        zeros); x0_next (K, nx): the next states (None: x1 + error of every tree that advances).  Needs the shift's maps
        (``BatchedMPC(controller)`` or ``qp.set_shift_maps``).  Returns dict cover, reopened (K each) -- or, with ``stats=False``,
        None and one synchronisation less.  Raises ``SearchTooBig``, with nothing changed, when the kept leaves outnumber the pool."""
        def state(a, name):
            if a is None:
                return None
            a = np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)
            if a.shape != (self.K, self.nx):
                raise ValueError('%s must have shape (%d, %d).' % (name, self.K, self.nx))
            return a
        e0, xn = state(errors, 'errors'), state(x0_next, 'x0_next')
        out = dict(cover=np.empty(self.K, dtype=np.int32), reopened=np.empty(self.K, dtype=np.int32)) if stats else None
        self._check(self.qp.lib.hmpc_search_advance(self._s, None if e0 is None else e0.ctypes.data, None if xn is None else xn.ctypes.data,
                                                    out['cover'].ctypes.data if stats else None, out['reopened'].ctypes.data if stats else None,
                                                    ctypes.c_void_p(stream)))
        self._B = self._P = 0
        return out

    def rebase(self, x0s, stats=True, stream=None):
        """The trees as they stand are carried to the states x0s (K, nx) of the same stage (``hmpc_search_rebase``): every alive
        node of a tree that has neither failed nor overflowed stays, its bound moved by -lam_0 . (x0_new - x0) of the dual row it
        carries; the other trees become their roots.  Running trees take part.  Needs no shift maps.  Returns dict cover,
        reopened (K each) -- or, with ``stats=False``, None and one synchronisation less.  Raises ``SearchTooBig``, with nothing
        changed, when the kept leaves outnumber the pool."""
        x0s = np.ascontiguousarray(np.atleast_2d(x0s), dtype=np.float64)
        if x0s.shape != (self.K, self.nx):
            raise ValueError('x0s must have shape (%d, %d).' % (self.K, self.nx))
        out = dict(cover=np.empty(self.K, dtype=np.int32), reopened=np.empty(self.K, dtype=np.int32)) if stats else None
        self._check(self.qp.lib.hmpc_search_rebase(self._s, x0s.ctypes.data, out['cover'].ctypes.data if stats else None,
                                                   out['reopened'].ctypes.data if stats else None, ctypes.c_void_p(stream)))
        self._B = self._P = 0
        return out

    def tree(self, k):
        """Tree k as it stands (for inspection): scalars and the whole slab, node_cap entries each (srow, sleft: the pool row
        of a node's waiting record or -1, the levels of waiting descendants below it)."""
        nc = self.node_cap
        sc, bd = np.empty(6, dtype=np.int32), np.empty(2)
        out = dict(fix=np.empty((nc, self.nfix), dtype=np.int8), lb=np.empty(nc), row=np.empty(nc, dtype=np.int32), wrow=np.empty(nc, dtype=np.int32),
                   alive=np.empty(nc, dtype=np.uint8))
        self._check(self.qp.lib.hmpc_search_tree(self._s, int(k), sc.ctypes.data, bd.ctypes.data, *[out[q].ctypes.data for q in ('fix', 'lb', 'row', 'wrow', 'alive')]))
        out.update(zip(('n', 'inc', 'inc_row', 'solves', 'uncertified', 'state'), (int(v) for v in sc)))
        out.update(ub=bd[0], unc_lb=bd[1], srow=np.empty(nc, dtype=np.int32), sleft=np.empty(nc, dtype=np.int32))
        self._check(self.qp.lib.hmpc_search_tree_waiting(self._s, int(k), out['srow'].ctypes.data, out['sleft'].ctypes.data))
        return out

    # ------------------------------------------------------------------
    def feedforward_many(self, x0s, warm_starts=None, frontier_width=8, tol=0., handdown=True, search_rule=None):
        """Solves K MIQPs; the list of dicts of ``BatchedMPC.feedforward_many`` (objective, ub, x, uc, leaves, solves, time,
        rounds).  ``x`` holds the two states the search returns (x0 and the model's next state), rows 0 and 1.
        search_rule: None (the search's rule as it is set) or ``best_first`` / ``depth_first`` / ``breadth_first`` of
        ``branch_and_bound.py`` -- the reference's ``candidate_selection`` -- which becomes the search's rule."""
        x0s = np.atleast_2d(np.asarray(x0s, dtype=np.float64))
        if search_rule is not None:
            self.set_rule(search_rule)
        tic = perf_counter()
        self.begin(x0s, warm_starts)
        rounds, _ = self.run(frontier_width, tol, handdown)
        r = self.results()
        t = perf_counter() - tic
        bad = r['state'] & (SEARCH_STATES['failed'] | SEARCH_STATES['overflow'])
        if np.any(bad & SEARCH_STATES['failed']):
            raise RuntimeError('QP solver did not converge on a node of %d searches' % int(((bad & SEARCH_STATES['failed']) != 0).sum()))
        if np.any(bad):
            raise RuntimeError('%d trees outgrew node_cap = %d' % (int((bad != 0).sum()), self.node_cap))
        leaves = self.leaves()
        nub = self.nfix // self.c.layout.T
        out = []
        for k in range(self.K):
            d = dict(objective=float(r['cost'][k]), ub=None, x=None, uc=None, leaves=leaves[k], solves=int(r['solves'][k]), time=t, rounds=rounds)
            if np.isfinite(r['cost'][k]):
                ub = r['binaries'][k].reshape(-1, nub).astype(np.float64)
                ub[0] = r['u0'][k, self.nu - nub:]                 # (stage 0 as the primal row has it: what the shift is given)
                d.update(x=np.stack((x0s[k], r['x1'][k])), uc=r['u0'][k:k + 1, :self.nu - nub].copy(), ub=ub)
            out.append(d)
        return out

    def _closed_loop_resident(self, x0s, n_steps, errors, frontier_width, tol, handdown, anytime=False):
        """``closed_loop`` with the trees, the pool and the step boundary on the device: ``begin`` once, then per step ``run`` ->
        ``results`` (K small rows) -> ``advance``.  A tree without an incumbent gets an empty cover and stays empty.
        anytime: the step's proven lower bounds and which trees their budget stopped are recorded too (``bounds``); a tree
        cut off with an incumbent advances like one that proved its optimum."""
        K = self.K
        stats = dict(nodes_ws=np.zeros((K, n_steps), np.int64), len_ws=np.zeros((K, n_steps), np.int64), reopened=np.zeros((K, n_steps), np.int64),
                     costs=np.full((K, n_steps), np.nan))
        if anytime:
            stats.update(lower=np.full((K, n_steps), np.nan), stopped=np.zeros((K, n_steps), bool))
        alive = np.ones(K, dtype=bool)
        tic = perf_counter()
        steps = 0
        self.begin(x0s)
        for t in range(n_steps):
            if not alive.any():
                break
            self.run(frontier_width, tol, handdown)
            r = self.results()
            bad = r['state'] & (SEARCH_STATES['failed'] | SEARCH_STATES['overflow'])
            if np.any(bad & SEARCH_STATES['failed']):
                raise RuntimeError('QP solver did not converge on a node of %d searches' % int(((bad & SEARCH_STATES['failed']) != 0).sum()))
            if np.any(bad):
                raise RuntimeError('%d trees outgrew node_cap = %d' % (int((bad != 0).sum()), self.node_cap))
            stats['nodes_ws'][alive, t] = r['solves'][alive]
            if anytime:
                stats['lower'][alive, t] = self.bounds(tol)['lower'][alive]
                stats['stopped'][alive, t] = (r['state'][alive] & SEARCH_STOP_STATES['budget']) != 0
            alive &= np.isfinite(r['cost'])
            if not alive.any():
                break
            a = self.advance(errors[:, t])
            stats['len_ws'][alive, t], stats['reopened'][alive, t], stats['costs'][alive, t] = a['cover'][alive], a['reopened'][alive], r['cost'][alive]
            steps += int(alive.sum())
        stats.update(steps=steps, wall=perf_counter() - tic)
        return stats

    def _raise_if_stopped(self, r):
        bad = r['state'] & (SEARCH_STATES['failed'] | SEARCH_STATES['overflow'])
        if np.any(bad & SEARCH_STATES['failed']):
            raise RuntimeError('QP solver did not converge on a node of %d searches' % int(((bad & SEARCH_STATES['failed']) != 0).sum()))
        if np.any(bad):
            raise RuntimeError('%d trees outgrew node_cap = %d' % (int((bad != 0).sum()), self.node_cap))

    def _closed_loop_presolve(self, x0s, n_steps, errors, frontier_width, tol, handdown):
        """``closed_loop`` with the search moved into the idle time between an input and the next measurement: after step t's
        ``results`` the trees ``advance`` to the PREDICTED state x1 (no error) and ``run`` there while the plant moves; on the
        measurement x1 + e_t they ``rebase`` and ``run`` again -- from a complete proof tree whose bounds moved by O(|e_t|) -- and
        only that second run and its ``results`` stand between the measurement and the input.  An idle-time search that stops
        FAILED or OVERFLOW costs nothing but its head start: the re-base makes such a tree its root."""
        K = self.K
        zeros = lambda: np.zeros((K, n_steps), np.int64)
        stats = dict(nodes_ws=zeros(), len_ws=zeros(), reopened=zeros(), costs=np.full((K, n_steps), np.nan), nodes_pre=zeros(), nodes_rt=zeros(),
                     reopened_rt=zeros(), rounds_rt=np.zeros(n_steps, np.int64), time_rt=np.zeros(n_steps), time_pre=np.zeros(n_steps))
        alive = np.ones(K, dtype=bool)
        xs = x0s.copy()
        tic = perf_counter()
        steps = 0
        if n_steps > 0:
            t0 = perf_counter()
            self.begin(xs)
            stats['rounds_rt'][0], _ = self.run(frontier_width, tol, handdown)
            r = self.results()
            stats['time_rt'][0] = perf_counter() - t0
            self._raise_if_stopped(r)
            stats['nodes_rt'][:, 0] = stats['nodes_ws'][:, 0] = r['solves']
        for t in range(n_steps):
            alive &= np.isfinite(r['cost'])
            if not alive.any():
                break
            t0 = perf_counter()
            a = self.advance(None)                                  # (to the model's next state: the measurement is not there yet)
            stats['len_ws'][alive, t], stats['reopened'][alive, t], stats['costs'][alive, t] = a['cover'][alive], a['reopened'][alive], r['cost'][alive]
            steps += int(alive.sum())
            if t + 1 == n_steps:
                break
            self.run(frontier_width, tol, handdown)                 # the idle-time search
            pre = self.results()
            stats['time_pre'][t + 1] = perf_counter() - t0
            xs[alive] = r['x1'][alive] + errors[alive, t]           # the measurement
            t0 = perf_counter()
            b = self.rebase(xs)
            stats['rounds_rt'][t + 1], _ = self.run(frontier_width, tol, handdown)
            r = self.results()
            stats['time_rt'][t + 1] = perf_counter() - t0
            self._raise_if_stopped(r)
            stats['nodes_pre'][alive, t + 1], stats['nodes_rt'][alive, t + 1], stats['reopened_rt'][alive, t + 1] = pre['solves'][alive], r['solves'][alive], b['reopened'][alive]
            stats['nodes_ws'][alive, t + 1] = pre['solves'][alive] + r['solves'][alive]
        stats.update(steps=steps, wall=perf_counter() - tic)
        return stats

    def closed_loop(self, x0, n_steps, errors, frontier_width=8, tol=0., handdown=True, resident=False, presolve=False, rule=None, max_solves=None):
        """K closed loops from the same x0 (or from K states, (K, nx)) under prescribed model errors (K, n_steps, nx), as
        ``FleetMPC.closed_loop``: per step ``run``, then the leaves go through the backend's node shift (``hmpc_shift_batch``) and
        become the covers of ``begin``.  ``resident=True``: the same walk with the step boundary on the device (``advance``) -- no
        leaf, identifier or dual row crosses the bus.
        ``presolve=True`` (implies the resident path): every step after the first is searched twice -- in the idle time at the
        model's predicted state, then, re-based to the measured one (``rebase``), again; see ``_closed_loop_presolve``.
        A loop whose MIQP is infeasible ends (its tree stays empty).  Returns dict of arrays (K, n_steps): nodes_ws, len_ws,
        reopened, costs (NaN where a loop has ended), steps, wall.  With ``presolve`` also nodes_pre (solves of the idle-time run),
        nodes_rt and rounds_rt (n_steps: solves and rounds after the re-base -- what the controller waits for; step 0: the cold
        search), reopened_rt (leaves the re-base reopened), time_pre and time_rt (n_steps, seconds: advance + idle-time run /
        re-base to results); nodes_ws is then nodes_pre + nodes_rt.
        ``rule`` / ``max_solves`` (resident path only; either one given): the loop runs under that rule and with that budget of
        solves per tree and step (``set_rule``, ``set_budget``; None: as the search is set), and the search has its own rule and
        budget again when the loop returns.  A step whose tree its budget stopped
        WITH an incumbent applies that incumbent's input and advances; one stopped without an incumbent ends its loop.  The dict
        gains lower (K, n_steps: the proven lower bound of every step's MIQP, NaN where a loop has ended) and stopped (K, n_steps,
        bool: the budget cut the step's search off)."""
        from .batched import BatchedMPC
        bm = BatchedMPC(self.c)                                 # (uploads the shift's maps)
        K = self.K
        errors = np.asarray(errors, dtype=np.float64)
        xs = np.asarray(x0, dtype=np.float64)
        xs = np.repeat(xs[None], K, axis=0) if xs.ndim == 1 else xs.copy()
        anytime = rule is not None or max_solves is not None
        if anytime and (presolve or not resident):
            raise ValueError('rule and max_solves need resident=True (and no presolve).')
        if presolve:
            return self._closed_loop_presolve(xs, n_steps, errors, frontier_width, tol, handdown)
        if resident:
            was = (self.rule, self.max_solves)
            try:
                if rule is not None:
                    self.set_rule(rule)
                if max_solves is not None:
                    self.set_budget(max_solves)
                return self._closed_loop_resident(xs, n_steps, errors, frontier_width, tol, handdown, anytime)
            finally:                                            # (the loop's rule and budget are the loop's: the search keeps its own)
                self.set_rule(was[0])
                self.set_budget(was[1])
        ws = None
        alive = np.ones(K, dtype=bool)
        nothing = NodeArrays(np.zeros((0, self.nfix), np.int8), np.zeros(0), np.zeros((0, self.n_dual)), np.zeros(0), np.zeros(0, bool))
        stats = dict(nodes_ws=np.zeros((K, n_steps), np.int64), len_ws=np.zeros((K, n_steps), np.int64), reopened=np.zeros((K, n_steps), np.int64),
                     costs=np.full((K, n_steps), np.nan))
        tic = perf_counter()
        steps = 0
        for t in range(n_steps):
            if not alive.any():
                break
            res = self.feedforward_many(xs, ws, frontier_width, tol, handdown)
            go = [k for k in range(K) if alive[k] and np.isfinite(res[k]['objective'])]
            for k in range(K):
                if alive[k]:
                    stats['nodes_ws'][k, t] = res[k]['solves']
            alive[:] = False
            alive[go] = True
            ws = [nothing] * K
            if not go:
                break
            new = bm.construct_warm_start_many([res[k]['leaves'] for k in go], xs[go],
                                               np.array([np.concatenate((res[k]['uc'][0], res[k]['ub'][0])) for k in go]), errors[go, t])
            for k, w in zip(go, new):
                ws[k] = w
                stats['len_ws'][k, t], stats['reopened'][k, t], stats['costs'][k, t] = len(w), int((~w.has_dual).sum()), res[k]['objective']
                xs[k] = res[k]['x'][1] + errors[k, t]
                steps += 1
        stats.update(steps=steps, wall=perf_counter() - tic)
        return stats
