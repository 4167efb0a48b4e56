"""The cases of tests/test_gpu_shipped_kernels.py: which built-in register kernel (``hmpc_kernel_info`` kind 2, one file each under
csrc/instances/) serves which horizon, and the nodes each of them is held to the oracle on.

The built-in kernels serve every host without a compiler and are the reference of both nets around a kernel compiled at run time
(first-use check, second opinion), while every other test of the suite runs the compiled ones.  Which instantiation serves follows
from the horizon through integer divisions of lanes by rows (``hmpc_static_slots``) and the lists of ``hmpc_pick_kernel``
(csrc/hmpc_kernel.hip); both are restated here, and the horizons of ``CASES`` sit on either side of every slot limit.

Nodes: the tree a cold branch and bound solves (helpers.real_tree_with_parents), each child with the row of its parent -- the
shape in which the parent -> child hand-down applies; at T <= 3, where that tree has 8 .. 24 nodes, 48 random prefixes beside it.
"""
import functools

import numpy as np

from helpers import load_fixture, make_controller, random_prefix_frontier, real_tree_with_parents

WALLS, ONE_WALL = 'cart_pole_with_walls', 'cart_pole_one_wall'
WAVE = 64
WAVES = (1, 2, 4)
# hmpc_pick_kernel: per shape (nx, nu, nub) the prefix of the instance files, the smallest wave count with a built-in kernel, and per
# wave count the (F, B, T) row slots of its instantiations in the order they are tried
BUILT_IN = {(4, 7, 4): ('c474', 1, {1: ((10, 3, 2),), 2: ((5, 2, 1), (10, 3, 1)), 4: ((3, 1, 1), (5, 2, 1))}),
            (4, 4, 2): ('c442', 2, {2: ((7, 2, 1),), 4: ((4, 1, 1),)})}
INSTANCES = tuple('%s_%d_%d_%d_w%d' % ((prefix,) + slots + (w,)) for prefix, _, tries in BUILT_IN.values() for w in sorted(tries) for slots in tries[w])
CASES = tuple((WALLS, T) for T in (2, 3, 20, 21, 27, 28, 40, 41, 45, 46)) + tuple((ONE_WALL, T) for T in (2, 42, 43, 52, 53))


def static_slots(nc, nub, nT, T, waves):
    """(kf, kb, kt) of hmpc_static_slots: slots per lane for the stage rows, the bounds of the binaries and the terminal set with
    ``waves`` wavefronts per node; None where a wavefront group cannot hold one stage."""
    nt = waves * WAVE
    if nc < 1 or nc > nt or nub < 1 or 2 * nub > nt:
        return None
    sp, sb = nt // nc, nt // (2 * nub)
    return (T + sp - 1) // sp, (T + sb - 1) // sb, (nT + nt - 1) // nt


def pick_kernel(nc, nub, nu, nT, T, waves, nx=4):
    """Name of the built-in instantiation hmpc_pick_kernel returns for ``waves`` waves asked, or None (the run-time-sized kernel
    serves).  The conditions on the problem's sparsity (static row map, at most 64 Gram entries, column length) hold for both
    cart-pole fixtures at every horizon; test_gpu_shipped_kernels.py asserts the outcome against hmpc_kernel_info."""
    if (nx, nu, nub) not in BUILT_IN:
        return None
    prefix, first, tries = BUILT_IN[nx, nu, nub]
    w = max(waves, first)
    while w <= 4:       # smallest instantiation that holds the rows; fewer waves than asked for never fit more rows
        slots = static_slots(nc, nub, nT, T, w)
        if slots is not None:
            for F, Bn, Tn in tries.get(w, ()):
                if slots[0] <= F and slots[1] <= Bn and slots[2] <= Tn:
                    return '%s_%d_%d_%d_w%d' % (prefix, F, Bn, Tn, w)
        w *= 2
    return None


def sizes(fixture):
    """(nc, nub, nu, nT) of a committed fixture: stage rows, binaries, inputs, terminal-set rows."""
    d = load_fixture(fixture)
    return d['F'].shape[0], int(d['nub']), d['B'].shape[1], d['F_T'].shape[0]


def choices(fixture, T):
    """The instantiation (or None) for 1, 2 and 4 waves asked."""
    nc, nub, nu, nT = sizes(fixture)
    return tuple(pick_kernel(nc, nub, nu, nT, T, w) for w in WAVES)


def _frozen(rec):
    for v in rec.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def nodes(fixture, T):
    """The nodes of a case and the oracle's records of them, computed once, shared, left unchanged: dict x0, fix [n], parent [n]
    (row of the parent, -1: none), tree (the first ``tree`` rows are the branch-and-bound tree), index [n] (the hand-down: parent
    where its record is optimal and polished), cold / handed (the oracle's records of the cold solve and of the solve with every
    child handed its parent's cold record), subset (rows of the full comparison), ctrl (the oracle's controller)."""
    ctrl = make_controller(fixture, T=T, backend='oracle', threads=8)
    x0 = np.array([0., 0., .5 if T <= 3 else 1., 0.])
    fix, parent = real_tree_with_parents(ctrl, x0)
    tree = len(fix)
    if T <= 3:
        extra = random_prefix_frontier(T, ctrl.mld.nub, 48, p_one=.1)
        extra[0, :] = -1
        fix, parent = np.vstack((fix, extra)), np.concatenate((parent, np.full(len(extra), -1, np.int32)))
    cold = _frozen(ctrl.qp.solve_batch(x0, fix))
    up = np.maximum(parent, 0)
    index = np.where((parent >= 0) & (cold['status'][up] == 0) & (cold['polished'][up] > 0), parent, -1).astype(np.int32)
    handed = _frozen(ctrl.qp.solve_batch(x0, fix, warm=(cold['primal'], cold['dual'], index)))
    rng = np.random.default_rng(1000 * T + len(fixture))
    each = 32 if T <= 3 else 16      # (the dense active-set solve of one optimal node takes 80 ms at T = 46)
    subset = np.sort(np.concatenate([rng.permutation(np.flatnonzero(cold['status'] == s))[:each] for s in (0, 1)]))
    for a in (fix, parent, index, subset):
        a.setflags(write=False)
    return dict(x0=x0, fix=fix, parent=parent, tree=tree, index=index, cold=cold, handed=handed, subset=subset, ctrl=ctrl)


def rows(rec, sel):
    """The records ``sel`` of a dict as solve_batch returns it."""
    n = len(rec['status'])
    return {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in rec.items()}


def terminal_parents(case, fixture, T):
    """Per node: its hand-down row holds a positive terminal-set multiplier (the order kernel's first bucket)."""
    nx, nc, nT = case['ctrl'].mld.nx, sizes(fixture)[0], sizes(fixture)[3]
    mu = case['cold']['dual'][:, (T + 1) * nx + T * nc:(T + 1) * nx + T * nc + nT]
    return (case['index'] >= 0) & (mu > 0).any(axis=1)[np.maximum(case['index'], 0)]


def tiled(n, B, seed):
    """B rows drawn from n distinct nodes so that every node occurs, under a seeded permutation."""
    return np.random.default_rng(seed).permutation(B) % n
