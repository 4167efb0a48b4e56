"""ctypes binding of the HIP library (``libhmpc.so``, C ABI in ``include/hmpc.h``).

This is the product path: there is no CPU fallback.  If the shared library is
missing, or no GPU is present, construction raises.  The library replaces the
reference's ``BoundedQP`` (a ``gurobipy.Model`` subclass,
``warm_start_hmpc/bounded_qp.py:5``) on the QP-relaxation path: where the
reference edits the right-hand sides of one Gurobi model per node and calls
``optimize`` (``controller.py:254-267``), ``solve_batch`` hands a whole
frontier of nodes to one kernel launch.
"""
import ctypes
import os
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# HMPC_LIBRARY_NAME selects a build variant next to the default one (diagnostic builds: libhmpc_stamps.so, A/B timing)
LIBRARY_PATH = os.path.join(os.path.dirname(_HERE), os.environ.get('HMPC_LIBRARY_NAME', 'libhmpc.so'))

STATUS_OPTIMAL, STATUS_INFEASIBLE, STATUS_MAXITER, STATUS_NUMERICAL = 0, 1, 2, 3

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


class _Problem(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ('nx', 'nu', 'nub', 'T', 'nc', 'ncT', 'nq', 'nr', 'nqT')] + \
               [(k, _dp) for k in ('A', 'B', 'F', 'G', 'h', 'F_Tm1', 'G_Tm1', 'h_Tm1', 'Q', 'R', 'Q_T')]


class _Options(ctypes.Structure):
    _fields_ = [('tol', ctypes.c_double), ('tol_inf', ctypes.c_double), ('max_iter', ctypes.c_int32),
                ('lazy_terminal', ctypes.c_int32), ('refine', ctypes.c_int32), ('device', ctypes.c_int32),
                ('polish', ctypes.c_int32), ('reserved', ctypes.c_int32), ('polish_tol', ctypes.c_double)]


class _Result(ctypes.Structure):
    _fields_ = [('obj', ctypes.c_void_p), ('dual_obj', ctypes.c_void_p), ('status', ctypes.c_void_p),
                ('iters', ctypes.c_void_p), ('primal', ctypes.c_void_p), ('dual', ctypes.c_void_p)]


class _Warm(ctypes.Structure):
    _fields_ = [('primal', ctypes.c_void_p), ('dual', ctypes.c_void_p), ('index', ctypes.c_void_p), ('rows', ctypes.c_int32)]


class _ShiftMaps(ctypes.Structure):
    _fields_ = [('M_mu', _dp), ('M_rho', _dp), ('V', _dp)]


class _CertTol(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ('polished', 'unpolished', 'infeasible', 'weak')]


class _BranchOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ('obj', 'word', 'pos', 'child_lb2', 'bits', 'child_offset', 'n_children',
                                               'child_fix', 'child_lb', 'child_parent', 'child_warm')]


# members of hmpc_branch_out, and the bits of its word (HMPC_BRANCH_* of include/hmpc.h)
BRANCH_OUTPUTS = tuple(k for k, _ in _BranchOut._fields_)
BRANCH_FLAGS = dict(branched=0x01, complete=0x02, pruned=0x04, infeasible=0x08, failed=0x10,
                    vertex=0x100, weak=0x200, uncertified=0x400, handed=0x800)


def iters_word(rec):
    """The ``iters`` word of the C ABI from a record dict of ``solve_batch``, which splits its flags off (polished, weak,
    handed, second, uncertified); a dict without those keys carries the word as it is."""
    iters = np.asarray(rec['iters']).astype(np.int64)
    for key, bit in (('polished', 0x10000), ('weak', 0x20000), ('handed', 0x40000), ('second', 0x80000), ('uncertified', 0x100000)):
        if rec.get(key) is not None:
            iters = (iters & ~bit) | np.where(np.asarray(rec[key]) > 0, bit, 0)
    return np.ascontiguousarray(iters, dtype=np.int32)


# columns of hmpc_certify_batch's residual matrix (HMPC_CERT_* of include/hmpc.h) and the classes of its verdict's low byte
CERT_COLUMNS = ('stationarity', 'sign', 'dual_obj', 'primal_equality', 'primal_inequality', 'obj', 'gap',
                'ray_quadratic', 'ray_objective', 'ray_primal')
CERT_CLASSES = ('polished', 'unpolished', 'infeasible', 'weak', 'skipped')
CERT_FAILED = 0x100


_lib = None


def load_library():
    """Loads libhmpc.so once; raises if it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is None:
        # A process has ONE HIP runtime: the first libamdhip64 loaded wins the soname.  PyTorch-ROCm ships its own copy;
        # if this library pulled in the system one first, a later torch.cuda initialisation finds "No HIP GPUs".  So
        # torch -- when it is installed -- goes first (it is what the device-pointer entry points are used with).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIBRARY_PATH):
            raise RuntimeError('HIP library %s not found: build it with __graft_entry__.build() '
                               '(make -C warm-start-hybrid-mpc_amd/csrc). There is no CPU fallback.' % LIBRARY_PATH)
        lib = ctypes.CDLL(LIBRARY_PATH)
        lib.hmpc_create.restype = ctypes.c_int
        lib.hmpc_create.argtypes = [ctypes.POINTER(_Problem), ctypes.POINTER(_Options), ctypes.POINTER(ctypes.c_void_p)]
        lib.hmpc_destroy.restype = ctypes.c_int
        lib.hmpc_destroy.argtypes = [ctypes.c_void_p]
        lib.hmpc_record_sizes.restype = ctypes.c_int
        lib.hmpc_record_sizes.argtypes = [ctypes.c_void_p, _ip, _ip]
        lib.hmpc_launch_info.restype = ctypes.c_int
        lib.hmpc_launch_info.argtypes = [ctypes.c_void_p, _ip, _ip]
        lib.hmpc_solve_batch.restype = ctypes.c_int
        lib.hmpc_solve_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                         ctypes.c_int32, ctypes.POINTER(_Warm), ctypes.POINTER(_Result)]
        lib.hmpc_solve_batch_device.restype = ctypes.c_int
        lib.hmpc_solve_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                ctypes.c_int32, ctypes.POINTER(_Warm), ctypes.POINTER(_Result), ctypes.c_void_p]
        lib.hmpc_last_error.restype = ctypes.c_char_p
        lib.hmpc_set_shift_maps.restype = ctypes.c_int
        lib.hmpc_set_shift_maps.argtypes = [ctypes.c_void_p, ctypes.POINTER(_ShiftMaps)]
        lib.hmpc_shift_batch.restype = ctypes.c_int
        lib.hmpc_shift_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 13
        lib.hmpc_shift_batch_device.restype = ctypes.c_int
        lib.hmpc_shift_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 14
        lib.hmpc_certify_batch.restype = ctypes.c_int
        lib.hmpc_certify_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                           ctypes.POINTER(_Result), ctypes.POINTER(_CertTol), ctypes.c_void_p, ctypes.c_void_p]
        lib.hmpc_certify_batch_device.restype = ctypes.c_int
        lib.hmpc_certify_batch_device.argtypes = lib.hmpc_certify_batch.argtypes + [ctypes.c_void_p]
        lib.hmpc_branch_batch.restype = ctypes.c_int
        lib.hmpc_branch_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(_Result), ctypes.c_void_p,
                                          ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_BranchOut)]
        lib.hmpc_branch_batch_device.restype = ctypes.c_int
        lib.hmpc_branch_batch_device.argtypes = lib.hmpc_branch_batch.argtypes + [ctypes.c_void_p]
        lib.hmpc_fleet_digest.restype = ctypes.c_int
        lib.hmpc_fleet_digest.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        lib.hmpc_fleet_create.restype = ctypes.c_int
        lib.hmpc_fleet_create.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
        lib.hmpc_fleet_destroy.restype = ctypes.c_int
        lib.hmpc_fleet_destroy.argtypes = [ctypes.c_void_p]
        lib.hmpc_fleet_reset.restype = ctypes.c_int
        lib.hmpc_fleet_reset.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        lib.hmpc_fleet_stop.restype = ctypes.c_int
        lib.hmpc_fleet_stop.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        lib.hmpc_fleet_rows.restype = ctypes.c_int
        lib.hmpc_fleet_rows.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        lib.hmpc_allreduce_incumbent_device.restype = ctypes.c_int
        lib.hmpc_allreduce_incumbent_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.hmpc_fleet_solve.restype = ctypes.c_int
        lib.hmpc_fleet_solve.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_double] + [ctypes.c_void_p] * 5
        lib.hmpc_fleet_shift.restype = ctypes.c_int
        lib.hmpc_fleet_shift.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.hmpc_fleet_uncertified.restype = ctypes.c_int
        lib.hmpc_fleet_uncertified.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        lib.hmpc_fleet_stats.restype = ctypes.c_int
        lib.hmpc_fleet_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        lib.hmpc_fleet_timing.restype = ctypes.c_int
        lib.hmpc_fleet_timing.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        lib.hmpc_fleet_handdown.restype = ctypes.c_int
        lib.hmpc_fleet_handdown.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]
        lib.hmpc_comm_unique_id.restype = ctypes.c_int
        lib.hmpc_comm_unique_id.argtypes = [ctypes.c_void_p]
        lib.hmpc_comm_create.restype = ctypes.c_int
        lib.hmpc_comm_create.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        lib.hmpc_allreduce_incumbent.restype = ctypes.c_int
        lib.hmpc_allreduce_incumbent.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
        lib.hmpc_publish_incumbent.restype = ctypes.c_int
        lib.hmpc_publish_incumbent.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_int32,
                                               ctypes.POINTER(ctypes.c_int32)]
        lib.hmpc_comm_destroy.restype = ctypes.c_int
        lib.hmpc_comm_destroy.argtypes = [ctypes.c_void_p]
        lib.hmpc_lp_solve_batch.restype = ctypes.c_int
        lib.hmpc_lp_solve_batch.argtypes = ([ctypes.c_int32] * 3 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                             ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_int32]
                                            + [ctypes.c_void_p] * 5)
        # the device-resident searches of include/hmpc_search.h
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        for name, args in (('hmpc_search_create', [vp, i32, i32, i32, ctypes.POINTER(vp)]), ('hmpc_search_destroy', [vp]),
                           ('hmpc_search_begin', [vp] * 7), ('hmpc_search_select', [vp, i32, ctypes.c_double, i32, _ip, vp]),
                           ('hmpc_search_batch', [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(_Warm), ctypes.POINTER(_Result), _ip]),
                           ('hmpc_search_put_records', [vp, i32, ctypes.POINTER(_Result)]), ('hmpc_search_consume', [vp, ctypes.c_double, vp]),
                           ('hmpc_search_run', [vp, i32, ctypes.c_double, i32, i32, vp, _ip, ctypes.POINTER(ctypes.c_int64)]),
                           ('hmpc_search_results', [vp] * 9), ('hmpc_search_leaves', [vp, _ip] + [vp] * 6),
                           ('hmpc_search_advance', [vp] * 6), ('hmpc_search_rebase', [vp] * 5),
                           ('hmpc_search_get_batch', [vp, i32] + [vp] * 5), ('hmpc_search_tree', [vp, i32] + [vp] * 7),
                           ('hmpc_search_rows', [vp, i32, i32, ctypes.POINTER(_Result), i32]),
                           ('hmpc_search_set_speculation', [vp, i32]), ('hmpc_search_staged', [vp, _ip, _ip]),
                           ('hmpc_search_counters', [vp, ctypes.POINTER(ctypes.c_int64)]), ('hmpc_search_tree_waiting', [vp, i32, vp, vp]),
                           # include/hmpc_search_anytime.h
                           ('hmpc_search_set_rule', [vp, i32]), ('hmpc_search_set_budget', [vp, i32, vp]),
                           ('hmpc_search_bounds', [vp, ctypes.c_double, vp, vp, vp, vp])):
            getattr(lib, name).restype = ctypes.c_int
            getattr(lib, name).argtypes = args
        _lib = lib
    return _lib


EXPORTED_SYMBOLS = ('hmpc_create', 'hmpc_destroy', 'hmpc_record_sizes', 'hmpc_launch_info', 'hmpc_kernel_info', 'hmpc_kernel_recipe', 'hmpc_jit_stats', 'hmpc_jit_build_problem', 'hmpc_validate_kernels', 'hmpc_second_opinion_review',
                    'hmpc_solve_batch', 'hmpc_solve_batch_device', 'hmpc_last_error',
                    'hmpc_set_shift_maps', 'hmpc_shift_batch', 'hmpc_shift_batch_device', 'hmpc_certify_batch', 'hmpc_certify_batch_device',
                    'hmpc_branch_batch', 'hmpc_branch_batch_device', 'hmpc_fleet_digest',
                    'hmpc_fleet_create', 'hmpc_fleet_destroy', 'hmpc_fleet_reset', 'hmpc_fleet_stop', 'hmpc_fleet_rows', 'hmpc_fleet_solve', 'hmpc_fleet_shift',
                    'hmpc_fleet_stats', 'hmpc_fleet_uncertified', 'hmpc_fleet_handdown', 'hmpc_fleet_timing', 'hmpc_comm_unique_id', 'hmpc_comm_create', 'hmpc_allreduce_incumbent', 'hmpc_allreduce_incumbent_device', 'hmpc_publish_incumbent', 'hmpc_comm_destroy',
                    'hmpc_lp_solve_batch')

# include/hmpc_search.h (a header of its own: include/hmpc.h is part of the key of every compiled kernel)
EXPORTED_SEARCH_SYMBOLS = ('hmpc_search_create', 'hmpc_search_destroy', 'hmpc_search_begin', 'hmpc_search_select', 'hmpc_search_batch',
                           'hmpc_search_put_records', 'hmpc_search_consume', 'hmpc_search_run', 'hmpc_search_results', 'hmpc_search_leaves',
                           'hmpc_search_advance', 'hmpc_search_rebase', 'hmpc_search_get_batch', 'hmpc_search_tree', 'hmpc_search_rows',
                           'hmpc_search_set_speculation', 'hmpc_search_staged', 'hmpc_search_counters', 'hmpc_search_tree_waiting')
SEARCH_STATES = dict(done=0x1, incumbent=0x2, failed=0x4, overflow=0x8)
# include/hmpc_search_anytime.h (a header of its own again: the two above name what include/hmpc_search.h declares, no more)
EXPORTED_SEARCH_ANYTIME_SYMBOLS = ('hmpc_search_set_rule', 'hmpc_search_set_budget', 'hmpc_search_bounds')
SEARCH_RULES = dict(best=0, depth=1, breadth=2, dive=3)
SEARCH_STOP_STATES = dict(budget=0x10)


def _problem_struct(problem):
    """``hmpc_problem`` of a ``problem_data()`` dict, and the arrays it points into (to be kept alive by the caller)."""
    keep = {}
    for k in ('A', 'B', 'F', 'G', 'F_Tm1', 'G_Tm1', 'Q', 'R', 'Q_T'):
        keep[k] = np.ascontiguousarray(np.atleast_2d(problem[k]), dtype=np.float64)
    for k in ('h', 'h_Tm1'):
        keep[k] = np.ascontiguousarray(problem[k], dtype=np.float64).reshape(-1)
    nx, nu, nub, T = int(problem['nx']), int(problem['nu']), int(problem['nub']), int(problem['T'])
    shapes = {'A': (nx, nx), 'B': (nx, nu), 'F': (keep['h'].size, nx), 'G': (keep['h'].size, nu),
              'F_Tm1': (keep['h_Tm1'].size, nx), 'G_Tm1': (keep['h_Tm1'].size, nu),
              'Q': (keep['Q'].shape[0], nx), 'R': (keep['R'].shape[0], nu), 'Q_T': (keep['Q_T'].shape[0], nx)}
    for k, shp in shapes.items():
        if keep[k].shape != shp:
            raise ValueError('Matrix %s has shape %s, expected %s.' % (k, keep[k].shape, shp))
    p = _Problem(nx=nx, nu=nu, nub=nub, T=T, nc=keep['h'].size, ncT=keep['h_Tm1'].size,
                 nq=keep['Q'].shape[0], nr=keep['R'].shape[0], nqT=keep['Q_T'].shape[0],
                 **{k: v.ctypes.data_as(_dp) for k, v in keep.items()})
    return p, keep


def jit_prebuild(problem):
    """Compiles (or finds in the cache) what ``hmpc_create`` would compile for ``problem`` -- without a GPU
    (``hmpc_jit_build_problem``): the kernels of the problem with its sizes as constants -- register kernels where the static
    row map holds the problem, the run-time-sized kernel or its streaming form elsewhere.  Returns the paths of the shared
    objects (none with ``HMPC_JIT_SIZED=0`` / ``HMPC_JIT=0``: the shipped kernels serve)."""
    lib = load_library()
    lib.hmpc_jit_build_problem.restype = ctypes.c_int
    lib.hmpc_jit_build_problem.argtypes = [ctypes.POINTER(_Problem), ctypes.POINTER(_Options), ctypes.c_char_p, ctypes.c_int32]
    p, keep = _problem_struct(problem)
    buf = ctypes.create_string_buffer(8192)
    if lib.hmpc_jit_build_problem(ctypes.byref(p), None, buf, 8192) != 0:
        raise RuntimeError('hmpc_jit_build_problem failed: %s' % lib.hmpc_last_error().decode())
    return [q for q in buf.value.decode().split('\n') if q]


def lp_solve_batch(A, c, b, relax=None, tol=1e-9, max_iter=100, device=-1):
    """The facet LPs of the offline terminal ingredients, one launch per sweep (``hmpc_lp_solve_batch``).

    maximise ``c_k'x`` s.t. ``A x <= b_k`` (+1 on row ``relax[k]``); ``c``: [n] or [B, n], ``b``: [m] or [B, m].
    Returns ``dict(obj[B], x[B, n], z[B, m], status[B], iters[B])``; status 0 optimal, 1 empty set, 4 unbounded.
    Replaces the Gurobi LP loops of ``mcais.py:103-118, 169-182`` and ``controller.py:205-226``.  Raises without the
    HIP library or a GPU: there is no CPU path.
    """
    lib = load_library()
    A = np.ascontiguousarray(A, dtype=np.float64)
    if A.ndim != 2:
        raise ValueError('lp_solve_batch: A must be a matrix')
    m, n = A.shape
    c = np.ascontiguousarray(c, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    B = max(c.shape[0] if c.ndim == 2 else 1, b.shape[0] if b.ndim == 2 else 1, 0 if relax is None else len(relax))
    if ((c.ndim == 2 and c.shape != (B, n)) or (c.ndim == 1 and c.size != n) or c.ndim > 2 or
            (b.ndim == 2 and b.shape != (B, m)) or (b.ndim == 1 and b.size != m) or b.ndim > 2):
        raise ValueError('lp_solve_batch: inconsistent sizes')
    rl = None
    if relax is not None:
        rl = np.ascontiguousarray(relax, dtype=np.int32)
        if rl.shape != (B,):
            raise ValueError('lp_solve_batch: relax must have one entry per LP')
    obj = np.empty(B); x = np.empty((B, n)); z = np.empty((B, m))
    status = np.empty(B, dtype=np.int32); iters = np.empty(B, dtype=np.int32)
    rc = lib.hmpc_lp_solve_batch(device, n, m, A.ctypes.data, c.ctypes.data, n if c.ndim == 2 else 0, b.ctypes.data,
                                 m if b.ndim == 2 else 0, rl.ctypes.data if rl is not None else None, B, tol, max_iter,
                                 obj.ctypes.data, x.ctypes.data, z.ctypes.data, status.ctypes.data, iters.ctypes.data)
    if rc != 0:
        raise RuntimeError('hmpc_lp_solve_batch failed (%d): %s' % (rc, lib.hmpc_last_error().decode()))
    return dict(obj=obj, x=x, z=z, status=status, iters=iters)


class HipBatchedQP(object):
    """Batched QP-relaxation solver on one MI355X.

    problem : dict as returned by ``HybridModelPredictiveController.problem_data()``
    tol, tol_inf, max_iter, lazy_terminal, refine, polish, polish_tol : see ``hmpc_options`` in include/hmpc.h
    device : HIP device ordinal (-1: current device)

    What a record owes these options (tests/test_solver_options.py): ``max_iter`` caps every pass of a
    node (two where the terminal set is tried lazily); a node left undecided (status >= 2) carries none of the flags ``polished``,
    ``weak``, ``uncertified``, ``handed``, and its rows and objectives are the last iterate's: they promise nothing.  An OPTIMAL record
    without ``polished`` met the stopping test on the SCALED cost: its relative gap is at most ``100 tol max(1, H)`` in the caller's
    units, H the largest entry of the cost's Hessian -- at the floor of the barrier parameter, an exit measured only without
    refinement (``refine=False``) and at ``tol=1e-10`` (include/hmpc.h, below ``hmpc_result``).  With ``polish=False`` nothing is handed down (``warm`` returns the cold records).
    """

    def __init__(self, problem, tol=1e-8, tol_inf=1e-6, max_iter=100, lazy_terminal=True, refine=True, device=-1,
                 polish=True, polish_tol=1e-4):
        self.lib = load_library()
        self.device = int(device)
        p, keep = _problem_struct(problem)
        nx, nu, nub, T = p.nx, p.nu, p.nub, p.T
        self._keep = keep
        o = _Options(tol=tol, tol_inf=tol_inf, max_iter=int(max_iter), lazy_terminal=int(bool(lazy_terminal)),
                     refine=int(bool(refine)), device=int(device), polish=int(bool(polish)), reserved=0,
                     polish_tol=float(polish_tol))
        handle = ctypes.c_void_p()
        rc = self.lib.hmpc_create(ctypes.byref(p), ctypes.byref(o), ctypes.byref(handle))
        if rc != 0:
            msg = self.lib.hmpc_last_error().decode()
            raise (ValueError if rc == -1 else RuntimeError)('hmpc_create failed (%d): %s' % (rc, msg))
        self.handle = handle
        n_primal, n_dual = ctypes.c_int32(), ctypes.c_int32()
        self.lib.hmpc_record_sizes(self.handle, ctypes.byref(n_primal), ctypes.byref(n_dual))
        self.n_primal, self.n_dual = n_primal.value, n_dual.value
        self.nx, self.nu, self.nfix, self._T = nx, nu, T * nub, T
        self._shift_ready = False

    def __del__(self):
        handle = getattr(self, 'handle', None)
        if handle:
            self.lib.hmpc_destroy(handle)
            self.handle = None

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError('hmpc call failed (%d): %s' % (rc, self.lib.hmpc_last_error().decode()))

    def lp_solve_batch(self, A, c, b, relax=None, **kw):
        """The facet LPs of the offline ingredients on this backend's device (see module-level ``lp_solve_batch``)."""
        return lp_solve_batch(A, c, b, relax=relax, device=self.device, **kw)

    def solve_batch(self, x0, fix, want_primal=True, want_dual=True, warm=None):
        """Host arrays in, host arrays out (copies included in ``time``).

        x0 : (nx,) shared or (B, nx); fix : int8 (B, T*nub), -1 free / 0 / 1
        warm : optional (primal rows, dual rows, index) -- the parent -> child hand-down of ``hmpc_warm``: node b tries
            the active set of the record in row ``index[b]`` of the two arrays (-1: none) before its first iteration
        """
        fix = np.ascontiguousarray(fix, dtype=np.int8)
        if fix.ndim != 2 or fix.shape[1] != self.nfix:
            raise ValueError('fix must have shape (B, %d).' % self.nfix)
        B = fix.shape[0]
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        if x0.shape == (self.nx,):
            stride = 0
        elif x0.shape == (B, self.nx):
            stride = self.nx
        else:
            raise ValueError('x0 must have shape (%d,) or (%d, %d).' % (self.nx, B, self.nx))
        out = dict(obj=np.empty(B), dual_obj=np.empty(B), status=np.empty(B, dtype=np.int32),
                   iters=np.empty(B, dtype=np.int32),
                   primal=np.empty((B, self.n_primal)) if want_primal else None,
                   dual=np.empty((B, self.n_dual)) if want_dual else None)
        res = _Result(**{k: (v.ctypes.data if v is not None else None) for k, v in out.items()})
        w = None
        if warm is not None:
            wp = np.ascontiguousarray(warm[0], dtype=np.float64).reshape(-1, self.n_primal)
            wd = np.ascontiguousarray(warm[1], dtype=np.float64).reshape(-1, self.n_dual)
            wi = np.ascontiguousarray(warm[2], dtype=np.int32)
            if wi.shape != (B,) or wp.shape[0] != wd.shape[0] or wi.max(initial=-1) >= wp.shape[0]:
                raise ValueError('warm: need (rows x n_primal, rows x n_dual, index of length B into the rows).')
            w = ctypes.byref(_Warm(wp.ctypes.data, wd.ctypes.data, wi.ctypes.data, wp.shape[0]))
        tic = time.perf_counter()
        self._check(self.lib.hmpc_solve_batch(self.handle, x0.ctypes.data, stride, fix.ctypes.data, B, w, ctypes.byref(res)))
        out['time'] = time.perf_counter() - tic
        out['handed'] = (out['iters'] >> 18) & 1        # HMPC_ITERS_HANDED: the active set handed down by the parent verified
        out['polished'] = (out['iters'] >> 16) & 1      # HMPC_ITERS_POLISHED
        out['weak'] = (out['iters'] >> 17) & 1          # HMPC_ITERS_WEAK: infeasible, the ray is no proof to tolerance
        out['uncertified'] = (out['iters'] >> 20) & 1   # HMPC_ITERS_UNCERTIFIED: weak, and pruned on the collapse of tau alone
        out['second'] = (out['iters'] >> 19) & 1        # HMPC_ITERS_TERMINAL: the terminal-set rows were needed (hand-down launches and the two-launch form)
        out['iters'] = out['iters'] & 0xFFFF
        return out

    def solve_batch_device(self, x0, fix, out, stream=None, warm=None, x0_stride=None):
        """Device-resident form: torch CUDA tensors in and out, asynchronous on ``stream``
        (default: torch's current stream).  ``out`` is a dict of preallocated tensors with keys
        obj, dual_obj (float64 [B]), status, iters (int32 [B]), primal [B, n_primal], dual [B, n_dual]
        (the last two may be None).  ``warm``: optional (primal rows, dual rows, int32 index [B]) CUDA tensors, the
        hand-down of ``hmpc_warm`` (the rows must not be rows of ``out``).  ``x0_stride``: doubles between the states of
        consecutive nodes in ``x0`` (the ``x0_stride`` of the C ABI: states inside wider rows); default 0 for one shared
        state, ``nx`` for a [B, nx] tensor."""
        import torch
        B = fix.shape[0]
        assert fix.dtype == torch.int8 and fix.is_cuda and fix.is_contiguous() and fix.shape[1] == self.nfix
        assert x0.dtype == torch.float64 and x0.is_cuda and x0.is_contiguous()
        stride = (0 if x0.dim() == 1 else self.nx) if x0_stride is None else int(x0_stride)
        assert x0.numel() >= max(0, (B - 1) * stride) + self.nx or 0 < stride < self.nx     # (a stride below nx the library refuses)
        res = _Result(**{k: (out[k].data_ptr() if out.get(k) is not None else None)
                         for k in ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual')})
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        w = None
        if warm is not None:
            wp, wd, wi = warm
            assert wp.is_cuda and wd.is_cuda and wi.is_cuda and wp.is_contiguous() and wd.is_contiguous() and wi.is_contiguous()
            assert wp.dtype == torch.float64 and wd.dtype == torch.float64 and wi.dtype == torch.int32 and wi.shape == (B,)
            assert wp.shape[1] == self.n_primal and wd.shape[1] == self.n_dual and wp.shape[0] == wd.shape[0]
            w = ctypes.byref(_Warm(wp.data_ptr(), wd.data_ptr(), wi.data_ptr(), wp.shape[0]))
        self._check(self.lib.hmpc_solve_batch_device(self.handle, x0.data_ptr(), stride, fix.data_ptr(), B, w,
                                                     ctypes.byref(res), ctypes.c_void_p(stream)))

    def jit_stats(self):
        """(compiled kernels dropped by the first-use check / the second opinion, solve calls in which the shipped kernel was
        asked for a second opinion, batches on which it ended like the compiled kernel) -- ``hmpc_jit_stats``; the counts of
        the last call are taken in first (``hmpc_second_opinion_review``: waits for them)."""
        self.lib.hmpc_second_opinion_review.restype = ctypes.c_int
        self.lib.hmpc_second_opinion_review.argtypes = [ctypes.c_void_p]
        self._check(self.lib.hmpc_second_opinion_review(self.handle))
        v = [ctypes.c_int32() for _ in range(3)]
        self.lib.hmpc_jit_stats.restype = ctypes.c_int
        self.lib.hmpc_jit_stats.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int32)] * 3
        self._check(self.lib.hmpc_jit_stats(self.handle, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def validate_kernels(self, x0, fix, stream=None):
        """Runs the first-use checks of the compiled kernels now (``hmpc_validate_kernels``; torch CUDA tensors as in
        ``solve_batch_device``) instead of inside the first solve call through each wave count."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        self.lib.hmpc_validate_kernels.restype = ctypes.c_int
        self.lib.hmpc_validate_kernels.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        self._check(self.lib.hmpc_validate_kernels(self.handle, x0.data_ptr(), 0 if x0.dim() == 1 else self.nx, fix.data_ptr(), fix.shape[0], ctypes.c_void_p(stream)))

    def kernel_recipe(self):
        """Per wave count (1 / 2 / 4 waves per node): 1 if the compiled kernel was built with the compiler's ILP schedule -- a binary
        listed in the cache's VALIDATED manifest --, 0 for the default schedule or a shipped kernel (``hmpc_kernel_recipe``)."""
        k = (ctypes.c_int32 * 3)()
        self.lib.hmpc_kernel_recipe.restype = ctypes.c_int
        self.lib.hmpc_kernel_recipe.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
        self._check(self.lib.hmpc_kernel_recipe(self.handle, k))
        return tuple(int(v) for v in k)

    def kernel_info(self):
        """Kind of kernel that serves this problem for 1 / 2 / 4 waves per node: 0 run-time-sized, 1 its streaming form,
        2 built-in register kernel, 4 / 5 / 6 the run-time-sized kernel / its streaming form / the register kernel compiled
        with this problem's sizes at creation (``hmpc_kernel_info``)."""
        k = (ctypes.c_int32 * 3)()
        self.lib.hmpc_kernel_info.restype = ctypes.c_int
        self.lib.hmpc_kernel_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
        self._check(self.lib.hmpc_kernel_info(self.handle, k))
        return tuple(int(v) for v in k)

    def launch_info(self):
        grid, lds = ctypes.c_int32(), ctypes.c_int32()
        self.lib.hmpc_launch_info(self.handle, ctypes.byref(grid), ctypes.byref(lds))
        return grid.value, lds.value

    # ------------------------------------------------------------------
    # warm-start node shift (controller.py:431-721 of the reference) on the device
    # ------------------------------------------------------------------
    def set_shift_maps(self, M_mu, M_rho, V):
        """Uploads the node-independent maps of the shift: mu'_{T-2} = M_mu mu_{T-1}, rho'_{T-1} = M_rho rho_T
        (``controller._update``) and the binary selector ``mld.V``."""
        keep = [np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64) for a in (M_mu, M_rho, V)]
        k = self._keep
        want = ((k['h'].size, k['h_Tm1'].size), (k['Q'].shape[0], k['Q_T'].shape[0]), (self.nfix // self._T, self.nu))
        for name, a, shp in zip(('M_mu', 'M_rho', 'V'), keep, want):
            if a.shape != shp:      # the library reads exactly these sizes from the host pointers
                raise ValueError('Matrix %s has shape %s, expected %s.' % (name, a.shape, shp))
        m = _ShiftMaps(*[a.ctypes.data_as(_dp) for a in keep])
        self._check(self.lib.hmpc_set_shift_maps(self.handle, ctypes.byref(m)))
        self._shift_ready = True

    def shift_batch(self, owner, x0, u0, e0, fix, lb, dual, dual_obj):
        """Shifts B leaves of K trees one stage (host arrays in and out).

        owner : int32 (B,) tree of each leaf;  x0, e0 : (K, nx);  u0 : (K, nu) applied inputs (uc, ub)
        fix : int8 (B, T*nub);  lb, dual_obj : (B,);  dual : (B, n_dual)
        Returns dict fix, lb, dual, dual_obj (B rows; rows of dropped leaves are undefined), keep (bool, B),
        reopened (bool, B), time.
        """
        if not self._shift_ready:
            raise RuntimeError('set_shift_maps has not been called')
        owner = np.ascontiguousarray(owner, dtype=np.int32)
        B = owner.size
        x0, u0, e0 = (np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64) for a in (x0, u0, e0))
        K = x0.shape[0]
        if x0.shape != (K, self.nx) or e0.shape != (K, self.nx) or u0.shape != (K, self.nu):
            raise ValueError('x0, e0 must be (K, nx) and u0 (K, nu).')
        fix = np.ascontiguousarray(fix, dtype=np.int8)
        lb, dual_obj = np.ascontiguousarray(lb, dtype=np.float64), np.ascontiguousarray(dual_obj, dtype=np.float64)
        dual = np.ascontiguousarray(dual, dtype=np.float64)
        if fix.shape != (B, self.nfix) or dual.shape != (B, self.n_dual) or lb.shape != (B,) or dual_obj.shape != (B,):
            raise ValueError('leaf arrays have inconsistent shapes.')
        if B and (owner.min() < 0 or owner.max() >= K):
            raise ValueError('owner out of range.')
        out = dict(fix=np.empty_like(fix), lb=np.empty(B), dual=np.empty_like(dual), dual_obj=np.empty(B))
        flags = np.zeros(B, dtype=np.uint8)
        tic = time.perf_counter()
        self._check(self.lib.hmpc_shift_batch(self.handle, B, K, owner.ctypes.data, x0.ctypes.data, u0.ctypes.data, e0.ctypes.data,
                                              fix.ctypes.data, lb.ctypes.data, dual.ctypes.data, dual_obj.ctypes.data,
                                              out['fix'].ctypes.data, out['lb'].ctypes.data, out['dual'].ctypes.data,
                                              out['dual_obj'].ctypes.data, flags.ctypes.data))
        out['time'] = time.perf_counter() - tic
        out['keep'] = (flags & 1).astype(bool)
        out['reopened'] = (flags & 2).astype(bool)
        return out

    def shift_batch_device(self, owner, x0, u0, e0, fix, lb, dual, dual_obj, out, stream=None):
        """Device-resident form: torch CUDA tensors; ``out`` is a dict of preallocated tensors fix (int8), lb, dual,
        dual_obj (float64) and flags (uint8: bit 0 keep, bit 1 reopened).  Asynchronous on ``stream``."""
        import torch
        if not self._shift_ready:
            raise RuntimeError('set_shift_maps has not been called')
        B, K = owner.shape[0], x0.shape[0]
        for t in (owner, x0, u0, e0, fix, lb, dual, dual_obj, out['fix'], out['lb'], out['dual'], out['dual_obj'], out['flags']):
            assert t.is_cuda and t.is_contiguous()
        assert owner.dtype == torch.int32 and fix.dtype == torch.int8 and out['flags'].dtype == torch.uint8
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        self._check(self.lib.hmpc_shift_batch_device(self.handle, B, K, owner.data_ptr(), x0.data_ptr(), u0.data_ptr(), e0.data_ptr(),
                                                     fix.data_ptr(), lb.data_ptr(), dual.data_ptr(), dual_obj.data_ptr(),
                                                     out['fix'].data_ptr(), out['lb'].data_ptr(), out['dual'].data_ptr(),
                                                     out['dual_obj'].data_ptr(), out['flags'].data_ptr(), ctypes.c_void_p(stream)))

    # ------------------------------------------------------------------
    # certificates of a batch of records (KKT point / Farkas ray) on the device
    # ------------------------------------------------------------------
    @staticmethod
    def _cert_tol(tol):
        if tol is None:
            return None
        return ctypes.byref(_CertTol(*[float(tol[k]) for k in ('polished', 'unpolished', 'infeasible', 'weak')]))

    def certify_batch(self, x0, fix, rec, tol=None):
        """Every record of ``rec`` (a dict as ``solve_batch`` returns it, all of obj, dual_obj, status, iters, primal, dual) held
        to its own certificate on the device (``hmpc_certify_batch``; host arrays in and out).

        x0, fix : as for ``solve_batch``;  tol : optional dict polished / unpolished / infeasible / weak (default 1e-8, 5e-6,
        1e-6, 1e-6).  Returns ``{name: float64 [B]}`` under the names of ``CERT_COLUMNS`` (NaN where a residual does not
        apply to the record's status), ``'class'`` (one of ``CERT_CLASSES`` per record), ``'failed'`` (bool) and
        ``'failed_mask'`` (bit c: column c of ``CERT_COLUMNS`` lies over its tolerance, or is NaN).
        """
        fix = np.ascontiguousarray(fix, dtype=np.int8)
        if fix.ndim != 2 or fix.shape[1] != self.nfix:
            raise ValueError('fix must have shape (B, %d).' % self.nfix)
        B = fix.shape[0]
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        if x0.shape == (self.nx,):
            stride = 0
        elif x0.shape == (B, self.nx):
            stride = self.nx
        else:
            raise ValueError('x0 must have shape (%d,) or (%d, %d).' % (self.nx, B, self.nx))
        # the iters word of the C ABI: solve_batch splits its flags off (a handed-down record of the oracle carries polished = 64)
        iters = np.asarray(rec['iters']).astype(np.int64) & 0xFFFF
        if rec.get('polished') is not None:
            iters |= np.where(np.asarray(rec['polished']) > 0, 0x10000, 0)
        if rec.get('weak') is not None:
            iters |= np.where(np.asarray(rec['weak']) > 0, 0x20000, 0)
        keep = dict(obj=np.ascontiguousarray(rec['obj'], dtype=np.float64), dual_obj=np.ascontiguousarray(rec['dual_obj'], dtype=np.float64),
                    status=np.ascontiguousarray(rec['status'], dtype=np.int32), iters=np.ascontiguousarray(iters, dtype=np.int32),
                    primal=np.ascontiguousarray(rec['primal'], dtype=np.float64), dual=np.ascontiguousarray(rec['dual'], dtype=np.float64))
        if keep['primal'].shape != (B, self.n_primal) or keep['dual'].shape != (B, self.n_dual) or \
                any(keep[k].shape != (B,) for k in ('obj', 'dual_obj', 'status', 'iters')):
            raise ValueError('record arrays have inconsistent shapes.')
        res = np.empty((B, len(CERT_COLUMNS)))
        verdict = np.empty(B, dtype=np.int32)
        r = _Result(**{k: v.ctypes.data for k, v in keep.items()})
        self._check(self.lib.hmpc_certify_batch(self.handle, x0.ctypes.data, stride, fix.ctypes.data, B, ctypes.byref(r),
                                                self._cert_tol(tol), res.ctypes.data, verdict.ctypes.data))
        out = {name: res[:, c].copy() for c, name in enumerate(CERT_COLUMNS)}
        out['class'] = np.array(CERT_CLASSES, dtype=object)[verdict & 0xFF]
        out['failed'] = (verdict & CERT_FAILED) != 0
        out['failed_mask'] = (verdict >> 16) & 0xFFFF
        return out

    def certify_batch_device(self, x0, fix, out, residuals, verdict, stream=None, tol=None):
        """Device-resident form: torch CUDA tensors, asynchronous on ``stream`` (default: torch's current stream).  ``out`` is
        exactly the dict ``solve_batch_device`` filled (all six tensors), so a solve followed by this call on one stream
        certifies a frontier without a host round trip.  residuals : float64 [B, 10] (columns: ``CERT_COLUMNS``);
        verdict : int32 [B] or None (low byte: index into ``CERT_CLASSES``, ``CERT_FAILED``, failing columns from bit 16)."""
        import torch
        B = fix.shape[0]
        assert fix.dtype == torch.int8 and fix.is_cuda and fix.is_contiguous() and fix.shape[1] == self.nfix
        assert x0.dtype == torch.float64 and x0.is_cuda and x0.is_contiguous()
        stride = 0 if x0.dim() == 1 else self.nx
        for k, dtype in (('obj', torch.float64), ('dual_obj', torch.float64), ('status', torch.int32), ('iters', torch.int32),
                         ('primal', torch.float64), ('dual', torch.float64)):
            assert out[k].is_cuda and out[k].is_contiguous() and out[k].dtype == dtype and out[k].shape[0] == B, k
        assert residuals.is_cuda and residuals.is_contiguous() and residuals.dtype == torch.float64 and residuals.shape == (B, len(CERT_COLUMNS))
        assert verdict is None or (verdict.is_cuda and verdict.is_contiguous() and verdict.dtype == torch.int32 and verdict.shape == (B,))
        res = _Result(**{k: out[k].data_ptr() for k in ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual')})
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        self._check(self.lib.hmpc_certify_batch_device(self.handle, x0.data_ptr(), stride, fix.data_ptr() if self.nfix else None, B,
                                                       ctypes.byref(res), self._cert_tol(tol), residuals.data_ptr(),
                                                       verdict.data_ptr() if verdict is not None else None, ctypes.c_void_p(stream)))

    # ------------------------------------------------------------------
    # branching a batch of solved nodes (controller.py:395-429 of the reference) on the device
    # ------------------------------------------------------------------
    def branch_batch(self, fix, rec, cutoff=None, warm_base=0, mark_weak=False, want=None):
        """The children of a batch of solved nodes, with their lower bounds (``hmpc_branch_batch``; host arrays in and out).

        fix : int8 (B, T*nub);  rec : a dict as ``solve_batch`` returns it (obj, status, iters, primal, dual; dual_obj with
        ``mark_weak``);  cutoff : optional (B,), a node whose objective is not below it is pruned;  warm_base : row of node 0 in
        the arrays the next solve is handed (``child_warm`` = warm_base + parent, -1 where the parent is no vertex);
        want : names of ``BRANCH_OUTPUTS`` to compute (default: all; the others are passed as NULL and are absent).
        Returns a dict of numpy arrays: obj, word (``BRANCH_FLAGS``), pos, child_lb2 (B, 2), bits (B, ceil(T*nub / 64)) uint64,
        child_offset, n_children (int), and the children, cut to n_children rows: child_fix, child_lb, child_parent,
        child_warm; with ``mark_weak`` also dual_obj, -inf on the weak nodes."""
        fix = np.ascontiguousarray(fix, dtype=np.int8)
        if fix.ndim != 2 or fix.shape[1] != self.nfix:
            raise ValueError('fix must have shape (B, %d).' % self.nfix)
        B = fix.shape[0]
        want = BRANCH_OUTPUTS if want is None else tuple(want)
        if set(want) - set(BRANCH_OUTPUTS):
            raise ValueError('want: unknown outputs %s' % sorted(set(want) - set(BRANCH_OUTPUTS)))
        keep = dict(obj=np.ascontiguousarray(rec['obj'], dtype=np.float64), status=np.ascontiguousarray(rec['status'], dtype=np.int32),
                    iters=iters_word(rec))
        for k, width in (('dual_obj', None), ('primal', self.n_primal), ('dual', self.n_dual)):
            if rec.get(k) is not None:
                keep[k] = np.array(rec[k], dtype=np.float64, order='C')     # (a copy: dual_obj is written with mark_weak)
                if keep[k].shape != ((B,) if width is None else (B, width)):
                    raise ValueError('record arrays have inconsistent shapes.')
        if any(keep[k].shape != (B,) for k in ('obj', 'status', 'iters')):
            raise ValueError('record arrays have inconsistent shapes.')
        if cutoff is not None:
            cutoff = np.ascontiguousarray(cutoff, dtype=np.float64)
            if cutoff.shape != (B,):
                raise ValueError('cutoff must have shape (B,).')
        words = (self.nfix + 63) // 64
        shapes = dict(obj=((B,), np.float64), word=((B,), np.int32), pos=((B,), np.int32), child_lb2=((B, 2), np.float64),
                      bits=((B, words), np.uint64), child_offset=((B,), np.int32), n_children=((1,), np.int32),
                      child_fix=((2 * B, self.nfix), np.int8), child_lb=((2 * B,), np.float64),
                      child_parent=((2 * B,), np.int32), child_warm=((2 * B,), np.int32))
        out = {k: np.zeros(shapes[k][0], dtype=shapes[k][1]) for k in want}
        r = _Result(**{k: v.ctypes.data for k, v in keep.items()})
        o = _BranchOut(**{k: v.ctypes.data for k, v in out.items()})
        self._check(self.lib.hmpc_branch_batch(self.handle, fix.ctypes.data, B, ctypes.byref(r), cutoff.ctypes.data if cutoff is not None else None,
                                               int(warm_base), int(bool(mark_weak)), ctypes.byref(o)))
        if 'n_children' in out:
            out['n_children'] = int(out['n_children'][0])
            for k in ('child_fix', 'child_lb', 'child_parent', 'child_warm'):
                if k in out:
                    out[k] = out[k][:out['n_children']]
        if mark_weak:
            out['dual_obj'] = keep['dual_obj']
        return out

    def branch_batch_device(self, fix, rec, out, cutoff=None, warm_base=0, mark_weak=False, stream=None):
        """Device-resident form: torch CUDA tensors, asynchronous on ``stream`` (default: torch's current stream).  ``rec`` is
        the dict ``solve_batch_device`` filled; ``out`` a dict of preallocated tensors under the names of ``BRANCH_OUTPUTS``
        (missing or None: not wanted) -- obj, child_lb2 [B, 2], child_lb [2B] float64; word, pos, child_offset [B], n_children
        [1], child_parent, child_warm [2B] int32; bits [B, ceil(T*nub / 64)] int64 (the words' bit patterns); child_fix
        [2B, T*nub] int8.  A solve, this call, and a solve of ``child_fix[:n_children]`` with ``child_warm`` as the hand-down
        index run on one stream without a row leaving the device."""
        import torch
        B = fix.shape[0]
        assert fix.dtype == torch.int8 and fix.is_cuda and fix.is_contiguous() and fix.shape[1] == self.nfix
        dtypes = dict(obj=torch.float64, child_lb2=torch.float64, child_lb=torch.float64, bits=torch.int64, child_fix=torch.int8)
        ptr = {}
        for k in BRANCH_OUTPUTS:
            t = out.get(k)
            if t is not None:
                assert t.is_cuda and t.is_contiguous() and t.dtype == dtypes.get(k, torch.int32), k
                assert t.shape[0] >= (1 if k == 'n_children' else 2 * B if k.startswith('child_') and k not in ('child_lb2', 'child_offset') else B), k
                ptr[k] = t.data_ptr()
        for k, dtype in (('obj', torch.float64), ('dual_obj', torch.float64), ('status', torch.int32), ('iters', torch.int32),
                         ('primal', torch.float64), ('dual', torch.float64)):
            assert rec.get(k) is None or (rec[k].is_cuda and rec[k].is_contiguous() and rec[k].dtype == dtype and rec[k].shape[0] >= B), k
        assert cutoff is None or (cutoff.is_cuda and cutoff.is_contiguous() and cutoff.dtype == torch.float64 and cutoff.shape == (B,))
        r = _Result(**{k: (rec[k].data_ptr() if rec.get(k) is not None else None) for k in ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual')})
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        self._check(self.lib.hmpc_branch_batch_device(self.handle, fix.data_ptr(), B, ctypes.byref(r), cutoff.data_ptr() if cutoff is not None else None,
                                                      int(warm_base), int(bool(mark_weak)), ctypes.byref(_BranchOut(**ptr)), ctypes.c_void_p(stream)))
