"""The warm-start node shift (csrc/hmpc_shift.hip: hmpc_shift_kernel<STAGED>, hmpc_shift_tree_kernel, hmpc_shift_row_kernel)
held to an extended-precision reference on the shapes the kernels branch on.

tests/shift_reference.py holds the reference, the derivation of every bound, the comparison and the workloads; this file
runs them.  The CPU half holds the product's float64 numpy form (``BatchedMPC.construct_warm_start``) to a QUARTER of each
bound a kernel gets -- which is what makes the bounds a comparison with the reference and not a tolerance --, checks that
every workload has leaves of every class on the reference alone, that the shifted objective of real multipliers is the
Lagrangian dual of the shifted row, and that the comparison refuses the defects these kernels could have.  The GPU half runs
both kernels (HMPC_SHIFT_ROWS unset: rows staged in LDS; 0: rows through registers) on the same workloads.

What the workloads reach that the cart-pole fixtures of tests/test_gpu_parity.py do not:
  * the persistent loop (prefetch one and two leaves ahead, reuse of a wave's LDS buffer, ragged last trip): the bench's own
    shift configuration, 65 536 synthetic leaves of 64 trees -- seventeen trips and a ragged eighteenth for the row kernel on
    256 CUs (15 waves per workgroup), sixteen for the register kernel;
  * row chunks past the first (nc = 38: two, nc = 84: three), `hmpc_shift_kernel<false>` and the fall-back of long rows to the
    register kernel (config4), identifiers past 192 binaries (config4: 240), nub = 3, 4, 8 and nuc = 2, 3, 6 in the retain
    rule, grids smaller than one workgroup's waves (1, 3, 4, 5, 63 leaves), a head of 232 rows (terminal set listed twice);
  * the device-pointer entry on a non-default torch stream, bit for bit beside the host-pointer one.
Every real-row workload produces leaves of all five classes (kept, dropped, finite bound, reopened, still infeasible); none is
unable to.  Not reached: nub = 0 or > 64, nx / nq / nr > 64, the fleet's row indirection (`src`), and more than one trip of
`hmpc_shift_kernel<false>` (three trips of config4's 35 KB rows are 0.9 GB of leaves).
"""
import functools

import numpy as np
import pytest

import shift_reference as sr

REAL_SPECS = tuple(sr.REAL)
CONFIG4 = (20, 6, 8, 0, 30)
BENCH = ('cart_pole_with_walls', 20)
SMALL = (1, 3, 4, 5, 63)
MINIMUM = dict(kept=20, dropped=5, finite=5, reopened=3, infeasible=3)


def bench_leaves(cus):
    """Every wave of the row kernel makes at least three trips and a ragged last one."""
    return max(3 * cus * 16 + 37, 65536)


@functools.lru_cache(maxsize=None)
def workload(name, cus=256):
    """(controller, workload, reference) by name: a spec of shift_reference.REAL, 'bench', ('small', B) or 'long_head'."""
    if name in sr.REAL:
        ctrl, w = sr.controller(name)[0], sr.real_workload(name)
    elif name == 'bench':
        ctrl = sr.controller(BENCH)[0]
        w = sr.synthetic_workload(ctrl, bench_leaves(cus), 64, seed=0)
    elif name == 'long_head':
        ctrl = sr.controller('long_head')[0]
        w = sr.synthetic_workload(ctrl, 600, 3, seed=2)
    else:
        ctrl = sr.controller(BENCH)[0]
        w = sr.synthetic_workload(ctrl, name[1], 3, seed=40 + name[1])
    return ctrl, w, sr.shift_reference_many(ctrl, w)


def _ids(v):
    return '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v)


ALL = REAL_SPECS + ('bench', 'long_head') + tuple(('small', B) for B in SMALL)


# ---- CPU half ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL, ids=_ids)
def test_numpy_form_within_a_quarter_of_each_bound(name):
    ctrl, w, ref = workload(name)
    got = sr.numpy_form_many(ctrl, w)
    c = sr.compare(ctrl, ref, got, factor=1.0)           # the bounds WITHOUT the factor 4 a kernel is allowed
    print('%s: numpy form, %s' % (_ids(name), c.figures()))
    assert c.ok, c.report()
    assert c.excluded <= 0.01 * c.kept
    counts = sr.class_counts(ref)
    print('%s: %s' % (_ids(name), counts))
    if isinstance(name, tuple) and name[0] == 'small':
        assert counts['kept'] >= 1 and counts['kept'] + counts['dropped'] == name[1]
    else:
        for what, least in MINIMUM.items():
            assert counts[what] >= least, (what, counts)


@pytest.mark.parametrize('name', REAL_SPECS, ids=_ids)
def test_shifted_objective_is_the_dual_objective_of_the_shifted_row(name):
    ctrl, w, ref = workload(name)
    lines, worst = sr.dual_objective_property(ctrl, w, ref, sr.numpy_form_many(ctrl, w))
    print('%s: |objective - dual objective| / (1 + |value|) at most %.3g' % (_ids(name), worst))
    assert not lines, '\n'.join(lines[:6])


def test_dispatch_arithmetic_of_the_shapes():
    # what hmpc_launch_shift decides, from the layout sizes alone: a change of the dispatch that moves a workload off the
    # kernel it is here to reach shows up as a failure of this test (and of its GPU twin below)
    lay = sr.controller(CONFIG4)[0].layout
    assert (lay.nc, lay.ncL, lay.T * lay.nub) == (84, 84, 240)
    assert sr.shift_lds_doubles(lay, True) * 8 > 64 * 1024 >= sr.shift_lds_doubles(lay, False) * 8    # 93 KB staged: maps read in place
    assert sr.shift_row_waves(lay) == 2                                                                # long rows: the register kernel
    assert sr.shift_dispatch(lay, 256, 480)[0] == sr.shift_dispatch(lay, 256, 480, rows=False)[0] == 'unstaged'
    lay = sr.controller((8, 3, 4, 2, 10))[0].layout
    assert (lay.nc, sr.shift_row_waves(lay)) == (38, 16)
    assert sr.shift_dispatch(lay, 256, 480) == ('row', 16, 30) and sr.shift_dispatch(lay, 256, 480, rows=False) == ('staged', 4, 120)
    lay = sr.controller(BENCH)[0].layout
    kernel, waves, grid = sr.shift_dispatch(lay, 256, bench_leaves(256))
    assert kernel == 'row' and bench_leaves(256) > 3 * grid * waves and bench_leaves(256) % (grid * waves) != 0
    kernel, waves, grid = sr.shift_dispatch(lay, 256, bench_leaves(256), rows=False)
    assert kernel == 'staged' and bench_leaves(256) > 3 * grid * waves
    lay = sr.controller('long_head')[0].layout
    assert lay.ncL == 232 > 192 and sr.shift_dispatch(lay, 256, 600, rows=False)[0] == 'staged'
    for B in SMALL:                                       # grid = need: fewer leaves than one workgroup has waves
        assert sr.shift_dispatch(lay := sr.controller(BENCH)[0].layout, 256, B)[2] == -(-B // sr.shift_row_waves(lay)) <= 5


def _as_result(ref):
    """A reference result in the shape of a kernel's: what a kernel without defect returns, to rounding."""
    return dict(keep=ref['keep'].copy(), reopened=ref['reopened'].copy(), fix=ref['fix'].copy(), lb=ref['lb'].copy(),
                dual=ref['dual'].copy(), dual_obj=ref['dobj'].copy())


def _with_objective(w, ref, raw):
    """... with another objective before the clip: clip, bound and reopen follow as in the kernels."""
    got = _as_result(ref)
    obj = np.maximum(raw, 0.)
    was_inf = np.isinf(w['lb'])
    got['dual_obj'] = obj
    got['reopened'] = was_inf & (obj <= 0.)
    got['lb'] = np.where(was_inf, np.where(got['reopened'], 0., w['lb']), obj)
    return got


def _mu0_rows_from_the_first_chunk(ctrl, w, ref):
    """Defect: the mu_0 term of rows r >= 32 multiplies row r - 32 of mu_0 (the prefetched first chunk used for every chunk)."""
    mld, cut = ctrl.mld, ctrl.layout.dual_slices()
    g = w['x0'].dot(mld.F.T) + w['u0'].dot(mld.G.T) - mld.h
    mu0 = w['dual'][:, cut['mu'][0]]
    nc = mu0.shape[1]
    delta = np.zeros(len(mu0))
    for r in range(32, nc):
        delta += (mu0[:, r] - mu0[:, r - 32]) * g[w['owner'], r]
    return _with_objective(w, ref, ref['obj_raw'].astype(np.float64) + delta)


def test_the_comparison_refuses_planted_defects():
    spec = (8, 3, 4, 2, 10)
    ctrl, w, ref = workload(spec)
    lay, cut = ctrl.layout, ctrl.layout.dual_slices()
    T = lay.T
    clean = sr.compare(ctrl, ref, _as_result(ref))
    assert clean.ok and clean.worst_map == clean.worst_obj == 0.

    # 1. the mu_0 term of rows r >= 32 taken from row r - 32: refused here (nc = 38) ...
    got = _mu0_rows_from_the_first_chunk(ctrl, w, ref)
    c = sr.compare(ctrl, ref, got)
    assert not c.ok and 'objective' in c.names(), c.report()
    assert sr.dual_objective_property(ctrl, w, ref, got)[0]                    # (and by the independent property)
    # ... and invisible on the cart-pole (nc = 28: there is no second chunk), which is all the older tests ran
    cp, wp, rp = workload(BENCH)
    assert cp.layout.nc == 28
    assert sr.compare(cp, rp, _mu0_rows_from_the_first_chunk(cp, wp, rp)).ok

    # 2. the tree vectors (F x0 + G u0 - h, Q x0, R u0, V u0) of the neighbouring tree: the owner of another trip
    other = dict(w, x0=np.roll(w['x0'], 1, axis=0), u0=np.roll(w['u0'], 1, axis=0))
    got = _with_objective(w, ref, sr.shift_reference_many(ctrl, other)['obj_raw'].astype(np.float64))
    c = sr.compare(ctrl, ref, got)
    assert 'objective' in c.names() and not set(c.names()) & {'copy', 'zero padding', 'fix', 'mapped mu', 'mapped rho', 'keep'}, c.report()
    assert sr.dual_objective_property(ctrl, w, ref, got)[0]

    # 3. identifier entries past 192 left unshifted (config4: 240 binaries)
    c4, w4, r4 = workload(CONFIG4)
    got = _as_result(r4)
    got['fix'][:, 192:] = w4['fix'][:, 192:]
    c = sr.compare(c4, r4, got)
    assert c.names() == ['fix'], c.report()
    assert 'stage 24' in c.report() or 'stage 2' in c.report()

    # 4. one padded zero not written
    got = _as_result(ref)
    b = int(np.flatnonzero(ref['keep'])[7])
    i = cut['sigma'][T - 1].start + 1
    got['dual'][b, i] = w['dual'][b, i] if w['dual'][b, i] != 0 else 1e-300
    c = sr.compare(ctrl, ref, got)
    assert c.names() == ['zero padding'], c.report()
    assert 'leaf %d ' % b in c.report() and '(sigma, stage %d, offset 1)' % (T - 1) in c.report()

    # 5. rho'_{T-1} left at zero
    got = _as_result(ref)
    got['dual'][:, cut['rho'][T - 1]] = 0.
    c = sr.compare(ctrl, ref, got)
    assert c.names() == ['mapped rho'], c.report()
    assert '(rho, stage %d' % (T - 1) in c.report()
    assert sr.dual_objective_property(ctrl, w, ref, got)[0]

    # (the report of a failing leaf names its trip of the persistent loop once the launch geometry is known)
    c = sr.compare(ctrl, ref, got, stride=64)
    assert '(trip %d)' % (int(np.flatnonzero(ref['keep'] & (np.abs(ref['dual'][:, cut['rho'][T - 1]]).sum(axis=1) > 0))[0]) // 64) in c.report(limit=1)


# ---- GPU half ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _backend(key):
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    ctrl = sr.controller(key)[0]
    qp = HipBatchedQP(ctrl.problem_data())
    qp.set_shift_maps(ctrl._update['mu'], ctrl._update['rho'], ctrl.mld.V)
    return qp


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _set_rows(monkeypatch, rows):
    if rows == 'unset':
        monkeypatch.delenv('HMPC_SHIFT_ROWS', raising=False)
    else:
        monkeypatch.setenv('HMPC_SHIFT_ROWS', rows)


def _hold(name, rows, ctrl, w, ref, got, real):
    kernel, waves, grid = sr.shift_dispatch(ctrl.layout, _cus(), len(w['owner']), rows=rows == 'unset')
    c = sr.compare(ctrl, ref, got, factor=4.0, stride=grid * waves)
    print('%s, HMPC_SHIFT_ROWS %s (%s kernel, %d workgroups of %d waves, %d trips): %s'
          % (_ids(name), rows, kernel, grid, waves, -(-len(w['owner']) // (grid * waves)), c.figures()))
    assert c.ok, c.report()
    if real:
        lines, worst = sr.dual_objective_property(ctrl, w, ref, got)
        print('%s, HMPC_SHIFT_ROWS %s: |objective - dual objective| / (1 + |value|) at most %.3g' % (_ids(name), rows, worst))
        assert not lines, '\n'.join(lines[:6])
    return kernel


def _shift(qp, w):
    return qp.shift_batch(w['owner'], w['x0'], w['u0'], w['e0'], w['fix'], w['lb'], w['dual'], w['dobj'])


# (config4's rows leave the row kernel two waves: HMPC_SHIFT_ROWS unset already runs the register kernel, there is no second kernel to run)
@pytest.mark.gpu
@pytest.mark.parametrize('name,rows', [(s, r) for s in REAL_SPECS for r in ('unset', '0') if (s, r) != (CONFIG4, '0')],
                         ids=lambda v: _ids(v))
def test_kernels_on_real_rows(monkeypatch, name, rows):
    _set_rows(monkeypatch, rows)
    ctrl, w, ref = workload(name)
    kernel = _hold(name, rows, ctrl, w, ref, _shift(_backend(name), w), real=True)
    if name == CONFIG4:
        lay = ctrl.layout
        assert sr.shift_lds_doubles(lay, True) * 8 > 64 * 1024 and sr.shift_row_waves(lay) == 2 and kernel == 'unstaged'
    else:
        assert kernel == ('row' if rows == 'unset' else 'staged')


@pytest.mark.gpu
@pytest.mark.parametrize('rows', ['unset', '0'])
def test_kernels_on_the_bench_configuration(monkeypatch, rows):
    # 65 536 leaves of 64 trees (more where 3 x CUs x 16 + 37 is more): every wave of the row kernel makes three trips and a ragged
    # last one.  Host-pointer entry and device-pointer entry on a non-default torch stream: the same bits.
    import torch
    _set_rows(monkeypatch, rows)
    ctrl, w, ref = workload('bench', _cus())
    assert len(w['owner']) == bench_leaves(_cus())
    qp = _backend(BENCH)
    got = _shift(qp, w)
    kernel = _hold('bench', rows, ctrl, w, ref, got, real=False)
    assert kernel == ('row' if rows == 'unset' else 'staged')
    dev = torch.device('cuda:0')
    t = {k: torch.from_numpy(w[k]).to(dev) for k in ('owner', 'x0', 'u0', 'e0', 'fix', 'lb', 'dual', 'dobj')}
    out = dict(fix=torch.zeros_like(t['fix']), lb=torch.zeros_like(t['lb']), dual=torch.zeros_like(t['dual']),
               dual_obj=torch.zeros_like(t['dobj']), flags=torch.zeros(len(w['owner']), device=dev, dtype=torch.uint8))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        qp.shift_batch_device(t['owner'], t['x0'], t['u0'], t['e0'], t['fix'], t['lb'], t['dual'], t['dobj'], out, stream=stream.cuda_stream)
    stream.synchronize()
    flags = out['flags'].cpu().numpy()
    keep = (flags & 1).astype(bool)
    np.testing.assert_array_equal(keep, got['keep'])
    np.testing.assert_array_equal((flags & 2).astype(bool)[keep], got['reopened'][keep])
    np.testing.assert_array_equal(out['fix'].cpu().numpy()[keep], got['fix'][keep])
    for k in ('lb', 'dual', 'dual_obj'):                  # bit for bit (rows of dropped leaves are undefined in both)
        a, b = out[k].cpu().numpy()[keep], got[k][keep]
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), k


@pytest.mark.gpu
@pytest.mark.parametrize('rows', ['unset', '0'])
@pytest.mark.parametrize('B', SMALL)
def test_kernels_on_batches_smaller_than_a_workgroup(monkeypatch, B, rows):
    _set_rows(monkeypatch, rows)
    ctrl, w, ref = workload(('small', B))
    _hold(('small', B), rows, ctrl, w, ref, _shift(_backend(BENCH), w), real=False)


@pytest.mark.gpu
@pytest.mark.parametrize('rows', ['unset', '0'])
def test_kernels_on_a_head_longer_than_one_batch(monkeypatch, rows):
    _set_rows(monkeypatch, rows)
    ctrl, w, ref = workload('long_head')
    assert ctrl.layout.ncL == 232
    _hold('long_head', rows, ctrl, w, ref, _shift(_backend('long_head'), w), real=False)
