"""hmpc_certify_batch on the device (csrc/hmpc_certify.hip), held to the extended-precision reference of
tests/certify_reference.py -- the same bound, workloads and planted defects as the CPU form in tests/test_certify_host.py."""
import numpy as np
import pytest

import certify_reference as cr
from certify_reference import COLUMNS, FAILED, WORKLOADS

pytestmark = pytest.mark.gpu
_BACKENDS = {}


def _hip(ctrl):
    """The product backend of a controller's problem (one handle per problem)."""
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    if id(ctrl) not in _BACKENDS:
        _BACKENDS[id(ctrl)] = (ctrl, HipBatchedQP(ctrl.problem_data()))
    return _BACKENDS[id(ctrl)][1]


def _fresh(ctrl, monkeypatch, stage):
    """A handle whose kernel form is capped by HMPC_CERTIFY_STAGE (a test switch hmpc_create reads): '1' rows in place, '0' matrices too."""
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    if stage == 'default':
        return _hip(ctrl)
    monkeypatch.setenv('HMPC_CERTIFY_STAGE', stage)
    return HipBatchedQP(ctrl.problem_data())


def _matrix(out):
    """(residuals [n, 10], verdict [n]) from the dict certify_batch returns."""
    from warm_start_hmpc_amd.qp_backend import CERT_CLASSES
    res = np.stack([out[k] for k in COLUMNS], axis=1)
    cls = np.array([CERT_CLASSES.index(k) for k in out['class']], dtype=np.int32)
    assert np.array_equal(out['failed'], out['failed_mask'] != 0)
    return res, (cls | np.where(out['failed'], FAILED, 0) | (out['failed_mask'].astype(np.int32) << 16)).astype(np.int32)


@pytest.mark.parametrize('name', WORKLOADS)
def test_oracle_records_within_the_bound_of_the_extended_reference(name):
    ctrl, x0, fix, rec, ref = cr.workload(name)
    res, verdict = _matrix(_hip(ctrl).certify_batch(x0, fix, rec))
    cr.compare(ref, res, verdict, what=name, show=True)
    left_out = cr.compare_verdicts(ref, verdict, what=name)                  # the verdict at the default tolerances
    print('%s: %d records, %d left out of the verdict comparison' % (name, len(verdict), left_out))


@pytest.mark.parametrize('which', ['cart_pole_n20', 'random_mld'])
def test_planted_defects_are_caught_with_the_same_mask(which):
    ctrl, x0, fix, rec, labels, want = cr.faulty_batches()[which]
    out = _hip(ctrl).certify_batch(x0, fix, rec)
    for i, (label, names) in enumerate(zip(labels, want)):
        assert out['failed'][i], label
        assert cr.names_of(out['failed_mask'][i]) == [k for k in COLUMNS if k in names], (label, cr.names_of(out['failed_mask'][i]), names)


def _device_call(qp, x0, fix, rec, B, idx):
    """certify_batch_device on rows ``idx`` of a workload's records, with a guard row behind the outputs."""
    import torch
    dev = torch.device('cuda', 0)
    t = lambda a, dtype: torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)
    out = dict(obj=t(rec['obj'][idx], torch.float64), dual_obj=t(rec['dual_obj'][idx], torch.float64), status=t(rec['status'][idx], torch.int32),
               iters=t(cr.iters_word(rec)[idx], torch.int32), primal=t(rec['primal'][idx], torch.float64), dual=t(rec['dual'][idx], torch.float64))
    res = torch.full((B + 1, len(COLUMNS)), -7., dtype=torch.float64, device=dev)
    verdict = torch.full((B + 1,), -7, dtype=torch.int32, device=dev)
    qp.certify_batch_device(t(x0, torch.float64), t(fix[idx], torch.int8), out, res[:B], verdict[:B])
    torch.cuda.synchronize()
    return res.cpu().numpy(), verdict.cpu().numpy()


@pytest.mark.parametrize('B', [1, 3, 257])
def test_batch_sizes_below_and_across_a_workgroup(B):
    # fewer records than a workgroup holds, and a count that is no multiple of it: every output row written, nothing behind the last
    ctrl, x0, fix, rec, ref = cr.workload('cart_pole_t10')
    idx = np.arange(B) % len(fix)
    res, verdict = _device_call(_hip(ctrl), x0, fix, rec, B, idx)
    assert np.all(res[B] == -7.) and verdict[B] == -7
    assert not np.any(res[:B] == -7.) and not np.any(verdict[:B] == -7)
    whole, whole_verdict = _matrix(_hip(ctrl).certify_batch(x0, fix, rec))
    assert np.array_equal(res[:B], whole[idx], equal_nan=True) and np.array_equal(verdict[:B], whole_verdict[idx])
    cr.compare(ref, whole, whole_verdict, what='cart_pole_t10')


def test_an_empty_batch_is_ok_and_writes_nothing():
    import ctypes
    import torch
    from warm_start_hmpc_amd.qp_backend import _Result
    ctrl, x0, fix, rec, ref = cr.workload('cart_pole_t10')
    qp = _hip(ctrl)
    res, verdict = _device_call(qp, x0, fix, rec, 0, np.arange(0))             # B == 0 through the binding: nothing raised ...
    assert np.all(res == -7.) and np.all(verdict == -7)                         # ... and the guard row untouched
    arrays = dict(obj=np.zeros(1), dual_obj=np.zeros(1), status=np.zeros(1, np.int32), iters=np.zeros(1, np.int32),
                  primal=np.zeros((1, qp.n_primal)), dual=np.zeros((1, qp.n_dual)))
    r = _Result(**{k: v.ctypes.data for k, v in arrays.items()})
    out, word = np.full((1, len(COLUMNS)), -7.), np.full(1, -7, np.int32)
    fix0 = np.ascontiguousarray(fix[:1])
    assert qp.lib.hmpc_certify_batch(qp.handle, x0.ctypes.data, 0, fix0.ctypes.data, 0, ctypes.byref(r), None, out.ctypes.data, word.ctypes.data) == 0
    assert np.all(out == -7.) and word[0] == -7
    assert qp.lib.hmpc_certify_batch(qp.handle, x0.ctypes.data, 0, fix0.ctypes.data, -1, ctypes.byref(r), None, out.ctypes.data, word.ctypes.data) == -1
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def config4():
    import test_certificates as tc
    ctrl, x0, fix = tc._config4_workload(16)
    rec = ctrl.qp.solve_batch(x0, fix)
    return ctrl, x0, fix, rec, cr.Reference(ctrl, x0, fix, rec)


@pytest.mark.parametrize('stage', ['default', '1', '0'])
def test_config4_with_matrices_staged_and_in_place(config4, monkeypatch, stage):
    # nx = 20, nu = 14, T = 30: 44 KB per record -- the rows stay in global memory, the matrices go to LDS (default, '1') or are
    # read in place ('0': what a problem whose matrices exceed the staging takes)
    ctrl, x0, fix, rec, ref = config4
    assert (ctrl.layout.nx, ctrl.layout.nu, ctrl.T) == (20, 14, 30) and len(fix) == 16
    res, verdict = _matrix(_fresh(ctrl, monkeypatch, stage).certify_batch(x0, fix, rec))
    cr.compare(ref, res, verdict, what='config4 stage ' + stage, show=True)
    cr.compare_verdicts(ref, verdict, what='config4')


@pytest.mark.parametrize('stage', ['1', '0'])
def test_rows_and_matrices_read_in_place_on_odd_sizes(monkeypatch, stage):
    # the forms a small problem never takes by itself, on the workload with odd sizes
    ctrl, x0, fix, rec, ref = cr.workload('random_mld_odd')
    res, verdict = _matrix(_fresh(ctrl, monkeypatch, stage).certify_batch(x0, fix, rec))
    cr.compare(ref, res, verdict, what='random_mld_odd stage ' + stage)


@pytest.mark.parametrize('T', [10, 20])
def test_solve_then_certify_on_one_stream_without_a_host_round_trip(T):
    import torch
    from helpers import make_controller, random_prefix_frontier
    from certificates import record_from_device
    hip = make_controller('cart_pole_with_walls', T=T, backend='hip')
    qp, dev = hip.qp, torch.device('cuda', 0)
    x0 = np.array([0., 0., .5, 0.])
    fix = random_prefix_frontier(T, 4, 64, p_one=0.1)
    fix[0, :] = -1
    B = len(fix)
    d_x0, d_fix = torch.tensor(x0, device=dev), torch.tensor(fix, device=dev)
    out = dict(obj=torch.empty(B, dtype=torch.float64, device=dev), dual_obj=torch.empty(B, dtype=torch.float64, device=dev),
               status=torch.empty(B, dtype=torch.int32, device=dev), iters=torch.empty(B, dtype=torch.int32, device=dev),
               primal=torch.empty((B, qp.n_primal), dtype=torch.float64, device=dev), dual=torch.empty((B, qp.n_dual), dtype=torch.float64, device=dev))
    res = torch.empty((B, len(COLUMNS)), dtype=torch.float64, device=dev)
    verdict = torch.empty(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        qp.solve_batch_device(d_x0, d_fix, out, stream=stream.cuda_stream)
        qp.certify_batch_device(d_x0, d_fix, out, res, verdict, stream=stream.cuda_stream)
    stream.synchronize()
    rec = record_from_device(*[out[k].cpu().numpy() for k in ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual')])
    rec['iters'] = out['iters'].cpu().numpy()
    assert (rec['status'] == 0).sum() >= 3 and (rec['status'] == 1).sum() >= 20 and (rec['status'] > 1).sum() == 0    # (both kinds of certificate)
    host, host_verdict = _matrix(qp.certify_batch(x0, fix, rec))
    assert np.array_equal(res.cpu().numpy(), host, equal_nan=True) and np.array_equal(verdict.cpu().numpy(), host_verdict)   # bit for bit
    cr.compare(cr.Reference(hip, x0, fix, rec), host, host_verdict, what='solve -> certify, T = %d' % T, show=True)
