"""hmpc_certify_batch without a GPU: the per-item arithmetic of csrc/hmpc_certify.h -- what the kernel's lanes run -- walked by a
serial host loop (tests/host/certify_driver.cpp) under AddressSanitizer and UBSan, held to the extended-precision reference of
tests/certify_reference.py on oracle records; the planted defects of test_certificates.py caught with the mask of failing
columns the host definition names; the C ABI's new entries: exported, rejecting bad arguments without a GPU, and no CPU answer
where there is none."""
import ctypes
import os

import numpy as np
import pytest

import certify_reference as cr
from certify_reference import COLUMNS, FAILED, WORKLOADS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    directory = tmp_path_factory.mktemp('certify')
    return cr.build_driver(directory), directory


@pytest.mark.parametrize('name', WORKLOADS)
def test_host_loop_matches_the_extended_reference(driver, name):
    ctrl, x0, fix, rec, ref = cr.workload(name)
    counts = np.bincount(ref.cls, minlength=5)
    assert counts[0] >= 4 and counts[4] == 0 and (counts[2] >= 10 or name == 'no_binaries'), counts
    res, verdict = cr.run_driver(*driver, ctrl, x0, fix, rec)
    cr.compare(ref, res, verdict, what=name, show=True)
    left_out = cr.compare_verdicts(ref, verdict, what=name)
    print('%s: %d records, %d left out of the verdict comparison' % (name, len(verdict), left_out))


@pytest.mark.parametrize('which', ['cart_pole_n20', 'random_mld'])
def test_planted_defects_fail_with_the_mask_of_the_host_definition(driver, which):
    ctrl, x0, fix, rec, labels, want = cr.faulty_batches()[which]
    assert len(labels) == (10 if which == 'random_mld' else 12 + 11)          # (PLANTED; ten single-residual faults, ray_primal in two forms)
    res, verdict = cr.run_driver(*driver, ctrl, x0, fix, rec)
    for label, v, names in zip(labels, verdict, want):
        assert names, label
        assert v & FAILED, label
        assert cr.names_of(v >> 16) == [k for k in COLUMNS if k in names], (label, cr.names_of(v >> 16), names)


def test_a_nan_in_a_dual_entry_fails_and_an_undecided_record_is_skipped(driver):
    ctrl, x0, fix, rec, ref = cr.workload('cart_pole_t10')
    opt = np.flatnonzero(rec['status'] == 0)[:3]
    r = {k: v[opt].copy() for k, v in rec.items() if isinstance(v, np.ndarray)}
    cut = ctrl.layout.dual_slices()
    r['dual'][0, cut['mu'][3].start + 5] = np.nan                   # one NaN among the multipliers of an optimal record
    r['status'][1] = 2                                              # an undecided node, whatever its rows hold
    r['dual'][1] = np.nan
    r['primal'][1] = np.nan
    res, verdict = cr.run_driver(*driver, ctrl, x0, fix[opt], r)
    host = cr.Reference(ctrl, x0, fix[opt], r)
    cr.compare(host, res, verdict)                                  # (NaN in the same columns as on the host)
    assert verdict[0] & FAILED and np.isnan(res[0, COLUMNS.index('stationarity')]) and np.isnan(res[0, COLUMNS.index('sign')])
    assert set(cr.names_of(verdict[0] >> 16)) >= {'stationarity', 'sign', 'dual_obj', 'gap'}
    assert verdict[1] == 4 and np.all(np.isnan(res[1]))             # class skipped, all NaN, not failed
    assert verdict[2] == 0 and np.all(np.isfinite(res[2, :7])) and np.all(np.isnan(res[2, 7:]))


def test_tolerances_are_an_argument(driver):
    # a stationarity residual between 1e-8 and 5e-6: fails as a polished record, passes as an unpolished one, and as a polished one
    # once `polished` lies above it
    ctrl, x0, fix, rec, ref = cr.workload('cart_pole_t10')
    i = np.flatnonzero(rec['status'] == 0)[1:2]
    r = {k: v[i].copy() for k, v in rec.items() if isinstance(v, np.ndarray)}
    r['dual'][0, ctrl.layout.dual_slices()['lam'][3].start] += 1e-7 * (1 + np.abs(r['dual'][0]).max())
    res, verdict = cr.run_driver(*driver, ctrl, x0, fix[i], r)
    assert 1e-8 < res[0, 0] < 5e-6
    assert verdict[0] & FAILED and cr.names_of(verdict[0] >> 16) == ['stationarity'] and verdict[0] & 0xFF == 0
    _, verdict = cr.run_driver(*driver, ctrl, x0, fix[i], r, tol=dict(cr.BASE, polished=2 * res[0, 0]))
    assert verdict[0] == 0
    _, verdict = cr.run_driver(*driver, ctrl, x0, fix[i], r, tol=dict(cr.BASE, polished=.5 * res[0, 0]))
    assert verdict[0] & FAILED
    r['polished'][0] = 0
    _, verdict = cr.run_driver(*driver, ctrl, x0, fix[i], r)
    assert verdict[0] == 1


def test_header_exports_and_binding_name_the_same_columns():
    import re
    from warm_start_hmpc_amd import qp_backend
    header = open(os.path.join(ROOT, 'include', 'hmpc.h')).read()
    cols = dict((name.lower(), int(v)) for name, v in re.findall(r'#define HMPC_CERT_([A-Z_]+)\s+(\d+)\b', header))
    assert cols.pop('count') == len(COLUMNS) and cols == {k: c for c, k in enumerate(COLUMNS)}
    assert qp_backend.CERT_COLUMNS == COLUMNS and qp_backend.CERT_CLASSES == cr.CLASS_NAMES
    assert {'hmpc_certify_batch', 'hmpc_certify_batch_device'} <= set(qp_backend.EXPORTED_SYMBOLS)
    lib = qp_backend.load_library()
    assert lib.hmpc_certify_batch is not None and lib.hmpc_certify_batch_device is not None


def test_invalid_arguments_are_rejected_without_touching_the_gpu():
    from warm_start_hmpc_amd.qp_backend import load_library, _Result
    lib = load_library()
    B = 2
    x0, fix, res = np.zeros(4), np.full((B, 40), -1, np.int8), np.zeros((B, 10))
    arrays = dict(obj=np.zeros(B), dual_obj=np.zeros(B), status=np.zeros(B, np.int32), iters=np.zeros(B, np.int32),
                  primal=np.zeros((B, 114)), dual=np.zeros((B, 560)))
    rec = _Result(**{k: v.ctypes.data for k, v in arrays.items()})
    for name, extra in (('hmpc_certify_batch', ()), ('hmpc_certify_batch_device', (None,))):
        fn = getattr(lib, name)

        def call(h=None, x=x0.ctypes.data, f=fix.ctypes.data, n=B, r=ctypes.byref(rec), out=res.ctypes.data):
            return fn(h, x, 0, f, n, r, None, out, None, *extra)
        assert call(n=-1) == -1 and b'batch size' in lib.hmpc_last_error()      # (HMPC_EINVAL, before anything is looked at)
        assert call(x=None) == -1 and b'null' in lib.hmpc_last_error()
        assert call(r=None) == -1 and call(out=None) == -1
        for k in arrays:                                                         # all six members of the records are required
            part = _Result(**{j: (v.ctypes.data if j != k else None) for j, v in arrays.items()})
            assert call(r=ctypes.byref(part)) == -1 and b'six members' in lib.hmpc_last_error(), k
        assert call() == -1 and b'null handle' in lib.hmpc_last_error()


@pytest.mark.skipif(_has_gpu(), reason='only meaningful on a box without a GPU')
def test_product_path_fails_loudly_without_gpu():
    # no handle without a device (HMPC_EDEVICE from hmpc_create, as for every other entry), and the binding has no CPU form
    from helpers import make_controller, _NoBackend
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP, load_library, _problem_struct
    data = make_controller('cart_pole_with_walls', T=10, backend=_NoBackend()).problem_data()
    p, keep = _problem_struct(data)
    handle = ctypes.c_void_p()
    assert load_library().hmpc_create(ctypes.byref(p), None, ctypes.byref(handle)) == -2 and not handle.value
    with pytest.raises(RuntimeError, match=r'\(-2\)'):
        HipBatchedQP(data)
