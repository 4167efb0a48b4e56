"""The built-in register kernels (``hmpc_kernel_info`` kind 2) as the SERVING kernels, and the hand-out of a launch.

Every other test of the suite runs the kernels compiled for its problem (tests/jit_problems.py pre-warms them; ``kernel_info() ==
(6, 6, 6)``), while the seven instantiations of csrc/instances/ serve every host without a compiler and are the reference of
the first-use check and of the second opinion.  Here they are created with ``HMPC_JIT=0`` -- the nets are off then, a record is
what the kernel itself returns -- and no test compiles anything.

A (no GPU)  tests/shipped_kernel_cases.py restates ``hmpc_static_slots`` and the lists of ``hmpc_pick_kernel``: the choices at
   the horizons of ``CASES`` are the listed ones, all seven instantiations occur, every slot limit is met from both sides, and
   the oracle's tree of every case holds the kinds of node the GPU part needs.
B  every case at 1 / 2 / 4 waves asked, cold and with every child handed its parent's cold record: statuses of the oracle on
   every node, objectives of every optimal node and the full ``test_gpu_parity._compare`` (dense active-set solve and certificates
   included) on a seeded subset, at that function's tolerances; cold records through the hand-down instantiation (all indices -1)
   equal to the cold kernel's to the bit.  Beyond the last built-in horizon the same is held on the run-time-sized kernel.
C  the hand-out of a launch (``hmpc_order_kernel`` from B > grid + grid / 8 on): batch sizes around that switch and around the
   kernel's 8192 nodes in registers, its byte path (a misaligned ``fix``, a problem with T nub % 4 != 0), its hand-down bucket,
   the order switched off; outputs filled with sentinels, none may be left, every record bit-equal to that of the same node in
   one small batch.  ``x0_stride`` > nx with NaN in the padding, and the refusal of a stride below nx.
"""
import contextlib
import os

import numpy as np
import pytest

import shipped_kernel_cases as sk
from shipped_kernel_cases import WALLS, ONE_WALL, CASES, WAVES

# the choices for 1 / 2 / 4 waves asked, from hmpc_pick_kernel and the fixtures' sizes (walls: nc = 28, nub = 4, nT = 102;
# one wall: nc = 19, nub = 2, nT = 8), by horizon range
LISTED = {WALLS: (((2, 20), ('c474_10_3_2_w1', 'c474_5_2_1_w2', 'c474_3_1_1_w4')),
                  ((21, 27), ('c474_10_3_1_w2', 'c474_10_3_1_w2', 'c474_3_1_1_w4')),
                  ((28, 40), ('c474_10_3_1_w2', 'c474_10_3_1_w2', 'c474_5_2_1_w4')),
                  ((41, 45), ('c474_5_2_1_w4',) * 3),
                  ((46, 64), (None,) * 3)),
          ONE_WALL: (((2, 42), ('c442_7_2_1_w2', 'c442_7_2_1_w2', 'c442_4_1_1_w4')),
                     ((43, 52), ('c442_4_1_1_w4',) * 3),
                     ((53, 64), (None,) * 3))}
ORDER_CASES = ((WALLS, 10), (ONE_WALL, 5))          # the workloads of part C
RECORD = ('obj', 'dual_obj', 'status', 'iters', 'primal', 'dual')
NAN_SENTINEL, INT_SENTINEL = 0x7ff80000dead0001, -7  # (a NaN that is not the 0x7ff8000000000000 of an infeasible node's primal row)
WORST = {}


def _listed(fixture, T):
    return next(names for (lo, hi), names in LISTED[fixture] if lo <= T <= hi)


# ---------------------------------------------------------------------------------------------------------------------------
# A. the cases are the right ones (no GPU)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fixture,T', CASES + ORDER_CASES)
def test_the_restated_choice_is_the_listed_one(fixture, T):
    assert sk.choices(fixture, T) == _listed(fixture, T)


def test_the_fixtures_have_the_sizes_the_list_was_derived_from():
    assert sk.sizes(WALLS) == (28, 4, 7, 102) and sk.sizes(ONE_WALL) == (19, 2, 4, 8)
    assert {(f, T) for f, T in CASES} == {(WALLS, T) for T in (2, 3, 20, 21, 27, 28, 40, 41, 45, 46)} | {(ONE_WALL, T) for T in (2, 42, 43, 52, 53)}
    for fixture, ranges in LISTED.items():           # the ranges tile 2 .. 64, and the restatement agrees inside them too
        assert [lo for (lo, _), _ in ranges] == [2] + [hi + 1 for (_, hi), _ in ranges[:-1]]
        for (lo, hi), names in ranges:
            for T in range(lo, hi + 1):
                assert sk.choices(fixture, T) == names, (fixture, T)


def test_all_seven_instantiations_occur_and_every_slot_limit_is_met_from_both_sides():
    assert len(sk.INSTANCES) == 7
    here = os.path.dirname(os.path.abspath(__file__))
    files = os.listdir(os.path.join(os.path.dirname(here), 'warm-start-hybrid-mpc_amd', 'csrc', 'instances'))
    assert sorted(f[:-4] for f in files if f.startswith('c4')) == sorted(sk.INSTANCES)
    served = {name for fixture, T in CASES for name in sk.choices(fixture, T)}
    assert served == set(sk.INSTANCES) | {None}
    # the stage-row slots kf decide every choice: for each instantiation (F slots, w waves) one case fills them (kf == F, it
    # serves) and one exceeds them by one (kf == F + 1, it does not serve)
    for name in sk.INSTANCES:
        fixture = WALLS if name.startswith('c474') else ONE_WALL
        F, Bn, Tn, w = (int(v) for v in name[5:].replace('w', '').split('_'))
        nc, nub, nu, nT = sk.sizes(fixture)
        kf = {T: sk.static_slots(nc, nub, nT, T, w)[0] for f, T in CASES if f == fixture}
        full, over = [T for T, k in kf.items() if k == F], [T for T, k in kf.items() if k == F + 1]
        assert full and over, (name, kf)
        assert all(name in sk.choices(fixture, T) for T in full) and not any(name in sk.choices(fixture, T) for T in over), name
        # the slots of the binaries' bounds (kb) and of the terminal set (kt) never decide at these sizes: wherever kf fits, they fit
        for T in range(2, 65):
            s = sk.static_slots(nc, nub, nT, T, w)
            assert s[0] > F or (s[1] <= Bn and s[2] <= Tn), (name, T, s)
    # ... and c474_10_3_2_w1 is the one whose terminal slots are exactly full (102 rows on 64 lanes)
    assert sk.static_slots(28, 4, 102, 20, 1) == (10, 3, 2)


@pytest.mark.parametrize('fixture,T', CASES + ORDER_CASES)
def test_the_oracles_tree_of_a_case_holds_what_the_kernels_are_held_on(fixture, T):
    c = sk.nodes(fixture, T)
    fix, parent, cold, tree = c['fix'], c['parent'], c['cold'], c['tree']
    nub = sk.sizes(fixture)[1]
    assert np.all(cold['status'] <= 1) and np.all(c['handed']['status'] <= 1)                    # the oracle decides every node
    assert np.array_equal(cold['status'], c['handed']['status'])
    n_opt, n_inf = int((cold['status'][:tree] == 0).sum()), int((cold['status'][:tree] == 1).sum())
    assert tree <= 370 and (len(fix) == tree) == (T > 3)
    if T >= 20:
        assert n_opt >= 50 and n_inf >= 50, (n_opt, n_inf)
    elif T <= 3:
        need = (7, 8) if fixture == WALLS else (5, 3)
        assert n_opt >= need[0] and n_inf >= need[1], (n_opt, n_inf)
    st = fix.reshape(len(fix), T, nub)
    assert ((st == 1).any(axis=2) & (st >= 0).all(axis=2)).any()       # a fully fixed stage that holds a one: the narrow stage body, constant direction
    assert int((parent[:tree] < 0).sum()) == 1 and np.all(parent[tree:] < 0) and np.all(parent < np.arange(len(fix)))
    assert np.all((c['index'] == parent) | (c['index'] == -1)) and (c['index'] >= 0).sum() >= tree // 2
    assert (c['handed']['polished'] == 64).any()                        # hand-downs that verify, on the oracle
    sub = c['subset']
    assert len(sub) <= 64 and (cold['status'][sub] == 0).sum() >= 8 and (cold['status'][sub] == 1).sum() >= 8


def test_the_order_workload_is_71_nodes_of_which_70_go_first():
    c = sk.nodes(WALLS, 10)
    assert len(c['fix']) == 71 and len(np.unique(c['fix'], axis=0)) == 71
    assert int(sk.terminal_parents(c, WALLS, 10).sum()) == 70           # children of a parent with a positive terminal-set multiplier
    assert (10 * 4) % 4 == 0 and (5 * 2) % 4 != 0                       # word path / byte path of the order kernel
    for B in (71, 2305, 9221):
        assert np.array_equal(np.unique(sk.tiled(71, B, 5)), np.arange(71))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(**values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update({k: str(v) for k, v in values.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_HANDLES = {}


def _qp(fixture, T, shipped=True):
    """One handle per problem, kept: the shipped kernels (HMPC_JIT=0 around the creation only) or the compiled ones."""
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    if (fixture, T, shipped) not in _HANDLES:
        with _env(HMPC_JIT=0) if shipped else contextlib.nullcontext():
            _HANDLES[fixture, T, shipped] = HipBatchedQP(sk.nodes(fixture, T)['ctrl'].problem_data())
    return _HANDLES[fixture, T, shipped]


def _to(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).to(torch.device('cuda', 0))


def _outputs(B, qp):
    """Output tensors of B records, every entry a sentinel."""
    import torch
    dev = torch.device('cuda', 0)
    out = {k: torch.full((B,) + ((getattr(qp, 'n_' + k),) if k in ('primal', 'dual') else ()), np.array(NAN_SENTINEL, np.uint64).view(np.int64).item(),
                         dtype=torch.int64, device=dev).view(torch.float64) for k in ('obj', 'dual_obj', 'primal', 'dual')}
    out.update({k: torch.full((B,), INT_SENTINEL, dtype=torch.int32, device=dev) for k in ('status', 'iters')})
    return out


def _bits(t):
    import torch
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _launch(qp, x0, fix, warm=None, x0_stride=None):
    """One launch of the device-pointer entry into outputs full of sentinels (tensors in, tensors out); no sentinel may be left."""
    import torch
    out = _outputs(fix.shape[0], qp)
    assert torch.isnan(out['obj']).all() and torch.isnan(out['dual']).all()
    qp.solve_batch_device(x0, fix, out, warm=warm, x0_stride=x0_stride)
    torch.cuda.synchronize()
    sentinel = np.array(NAN_SENTINEL, np.uint64).view(np.int64).item()
    for k in RECORD:
        left = int((_bits(out[k]) == (INT_SENTINEL if k in ('status', 'iters') else sentinel)).sum())
        assert left == 0, ('%d entries of %s were not written' % (left, k), fix.shape[0])
    return out


def _assert_same_bits(out, ref, rows=None, what=''):
    """Every array of ``out`` equal to the rows ``rows`` of ``ref`` to the bit (NaN payloads and signed zeros included)."""
    import torch
    for k in RECORD:
        want = ref[k] if rows is None else ref[k][rows]
        same = _bits(out[k]) == _bits(want)
        if not bool(same.all()):
            bad = torch.nonzero(~same.reshape(same.shape[0], -1).all(dim=1)).flatten()
            raise AssertionError('%s: %s differs in %d records, the first ones %s' % (what, k, len(bad), bad[:8].tolist()))


def _host(out):
    """Records of a launch as solve_batch returns them (flags split off the iters word)."""
    rec = {k: v.cpu().numpy() for k, v in out.items()}
    word = rec['iters']
    rec.update(handed=(word >> 18) & 1, polished=(word >> 16) & 1, weak=(word >> 17) & 1, uncertified=(word >> 20) & 1, second=(word >> 19) & 1, iters=word & 0xFFFF)
    return rec


# ---------------------------------------------------------------------------------------------------------------------------
# B. every built-in instantiation against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', autouse=True)
def _report_margins():
    """The deviations and certificate margins of THIS module's comparisons, printed the way tests/test_gpu_parity.py prints its
    own (whose tally is put back, with this module's figures taken in) and appended to the file HMPC_PARITY_MARGINS names, if set.
    They are figures, not bounds."""
    import test_gpu_parity as tp
    from certificates import new_margins, margins_line
    kept_worst, kept_margins = dict(tp.WORST), tp.MARGINS
    for k in tp.WORST:
        tp.WORST[k] = 0.
    tp.MARGINS = new_margins()
    yield
    mine, margins = dict(tp.WORST), tp.MARGINS
    for k in tp.WORST:
        tp.WORST[k] = max(kept_worst[k], mine[k])
    tp.MARGINS = kept_margins
    for cls, values in margins.items():
        for name, (value, reference) in values.items():
            seen = kept_margins[cls].setdefault(name, [0., 0.])
            seen[0], seen[1] = max(seen[0], value), max(seen[1], reference)
    if not WORST:
        return
    line = ('shipped kernels (kind 2, and the run-time-sized kernel beyond their horizons) vs oracle: objectives of all optimal nodes %.2e relative '
            '(%d nodes, %d of them with a verified hand-down); subsets norm-wise %.2e, element-wise %.2e; vs dense active-set solve %.2e; '
            'unpolished records norm-wise %.2e' % (WORST['obj'], WORST['nodes'], WORST['handed'], mine['norm'], mine['element'], mine['dense'], mine['iterate']))
    line += '; ' + margins_line(margins)
    print('\n' + line)
    if os.environ.get('HMPC_PARITY_MARGINS'):
        with open(os.environ['HMPC_PARITY_MARGINS'], 'a') as f:
            f.write(line + '\n')


@pytest.mark.gpu
@pytest.mark.parametrize('waves', WAVES)
@pytest.mark.parametrize('fixture,T', CASES)
def test_the_serving_shipped_kernel_returns_the_oracles_records(fixture, T, waves):
    from test_gpu_parity import _compare
    c = sk.nodes(fixture, T)
    qp, x0, fix, index, sub = _qp(fixture, T), c['x0'], c['fix'], c['index'], c['subset']
    want = sk.choices(fixture, T)
    if all(want):
        assert qp.kernel_info() == (2, 2, 2), qp.kernel_info()
    else:
        # beyond the last built-in horizon (walls T = 46, one wall T = 53): the run-time-sized kernel, lists and factor in LDS
        # (kind 0; 75 kB and 58 kB of LDS per node, far from the 160 kB at which its streaming form, kind 1, takes over)
        assert want == (None,) * 3 and qp.kernel_info() == (0, 0, 0), (want, qp.kernel_info())
    with _env(HMPC_WAVES=waves):
        cold = qp.solve_batch(x0, fix)
        assert np.array_equal(cold['status'], c['cold']['status']), np.flatnonzero(cold['status'] != c['cold']['status'])
        assert np.all(cold['polished'][index[index >= 0]] > 0)                     # (only polished optimal records are handed down)
        hand = qp.solve_batch(x0, fix, warm=(cold['primal'], cold['dual'], index))
        none = _launch(qp, _to(x0), _to(fix), warm=(_to(cold['primal']), _to(cold['dual']), _to(np.full(len(fix), -1, np.int32))))
    assert hand['handed'].sum() >= 1 and not np.any(hand['handed'][index < 0])
    for a, b, what in ((cold, c['cold'], 'cold'), (hand, c['handed'], 'hand-down')):
        assert np.array_equal(a['status'], b['status']), (what, np.flatnonzero(a['status'] != b['status']))
        fin = b['status'] == 0
        dev = np.max(np.abs(a['obj'][fin] - b['obj'][fin]) / np.abs(b['obj'][fin]))
        print('%s T = %d, %d waves asked (%s), %s: %d nodes, %d optimal, %d handed; objectives within %.2e of the oracle\'s'
              % (fixture, T, waves, want[WAVES.index(waves)], what, len(fix), fin.sum(), a['handed'].sum(), dev))
        WORST['obj'] = max(WORST.get('obj', 0.), dev)
        WORST['nodes'] = WORST.get('nodes', 0) + len(fix)
        WORST['handed'] = WORST.get('handed', 0) + int(a['handed'].sum())
        np.testing.assert_allclose(a['obj'][fin], b['obj'][fin], rtol=1e-8, atol=1e-11)      # (_compare's objective tolerance, on every node)
        _compare(c['ctrl'], sk.rows(a, sub), sk.rows(b, sub), T, fix[sub], x0=x0)
    # the hand-down instantiation with nothing handed: the cold kernel's records to the bit
    none = _host(none)
    assert not none['handed'].any()
    for k in RECORD + ('polished', 'weak', 'uncertified'):
        assert np.array_equal(np.asarray(none[k]).view(np.uint8), np.asarray(cold[k], dtype=none[k].dtype).view(np.uint8)), (k, 'hand-down instantiation, all indices -1')


# ---------------------------------------------------------------------------------------------------------------------------
# C. the hand-out of a launch
# ---------------------------------------------------------------------------------------------------------------------------
_SMALL = {}
SIZES = {'g': lambda g: g, 'g + 1': lambda g: g + 1, 'g + g // 8': lambda g: g + g // 8, 'g + g // 8 + 1': lambda g: g + g // 8 + 1,
         '8192': lambda g: 8192, '8193': lambda g: 8193, '9221': lambda g: 9221}


def _order_workload(fixture, T):
    """The handle (compiled kernels for the pre-warmed walls T = 10, shipped ones for one wall T = 5), its tree on the device, the
    records of the distinct nodes in ONE small batch under HMPC_WAVES=1 -- cold and with real-parent hand-down -- and the number
    of resident workgroups g of a large launch (hmpc_launch_info after a first large call)."""
    key = fixture, T
    if key not in _SMALL:
        c = sk.nodes(fixture, T)
        shipped = (fixture, T) != (WALLS, 10)
        qp = _qp(fixture, T, shipped)
        assert qp.kernel_info() == ((2, 2, 2) if shipped else (6, 6, 6)), qp.kernel_info()    # nothing compiles here
        x0, fix, index = _to(c['x0']), _to(c['fix']), _to(c['index'])
        with _env(HMPC_WAVES=1):
            cold = _launch(qp, x0, fix)
            warm = (cold['primal'], cold['dual'])
            hand = _launch(qp, x0, fix, warm=warm + (index,))
            big = sk.tiled(len(c['fix']), 9221, 0)
            _launch(qp, x0, fix[_to(big)])
            g = qp.launch_info()[0]
        status = cold['status'].cpu().numpy()
        assert np.array_equal(status, c['cold']['status']) and np.array_equal(hand['status'].cpu().numpy(), c['handed']['status'])
        assert ((hand['iters'].cpu().numpy() >> 18) & 1).sum() >= 1
        assert 64 <= g and g + g // 8 + 1 < 8192, g
        _SMALL[key] = dict(qp=qp, x0=x0, fix=fix, index=index, cold=cold, hand=hand, warm=warm, g=g, n=len(c['fix']))
    return _SMALL[key]


def _tiled_launch(w, B, seed, mode, fix_at=None, **env):
    """B nodes tiled from the workload under a seeded permutation, cold or with real-parent hand-down (index into the rows of the
    distinct nodes' cold records); every record must be that of the same node in the small batch, to the bit."""
    tile = _to(sk.tiled(w['n'], B, seed))
    fix = w['fix'][tile].contiguous()
    if fix_at is not None:
        fix = fix_at(fix)
    with _env(HMPC_WAVES=1, **env):
        out = _launch(w['qp'], w['x0'], fix, warm=w['warm'] + (w['index'][tile].contiguous(),) if mode == 'hand-down' else None)
        grid = w['qp'].launch_info()[0]
    assert grid == min(B, w['g'])
    _assert_same_bits(out, w['hand' if mode == 'hand-down' else 'cold'], tile, what='B = %d, %s' % (B, mode))
    return out


def _one_byte_in(fix):
    """The same entries, starting one byte into a larger buffer."""
    import torch
    buf = torch.full((fix.numel() + 8,), -1, dtype=torch.int8, device=fix.device)
    moved = buf[1:1 + fix.numel()].view(fix.shape)
    moved.copy_(fix)
    assert moved.data_ptr() % 4 == 1 and moved.is_contiguous()
    return moved


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['cold', 'hand-down'])
@pytest.mark.parametrize('size', list(SIZES))
def test_every_node_of_a_large_launch_is_handed_out_once(size, mode):
    w = _order_workload(WALLS, 10)
    B = SIZES[size](w['g'])
    _tiled_launch(w, B, 1 + B, mode)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['cold', 'hand-down'])
def test_the_order_switched_off_gives_the_same_bits(mode):
    _tiled_launch(_order_workload(WALLS, 10), 9221, 7, mode, HMPC_NO_ORDER=1)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['cold', 'hand-down'])
def test_the_order_kernel_counts_a_misaligned_fix_by_bytes(mode):
    w = _order_workload(WALLS, 10)
    _tiled_launch(w, w['g'] + w['g'] // 8 + 1, 11, mode, fix_at=_one_byte_in)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['cold', 'hand-down'])
@pytest.mark.parametrize('size', ['g + g // 8 + 1', '8193'])
def test_the_order_kernel_counts_rows_of_ten_entries_by_bytes(size, mode):
    w = _order_workload(ONE_WALL, 5)                 # T nub = 10: no multiple of four, shipped kernel c442_7_2_1_w2
    assert w['fix'].shape[1] == 10
    B = SIZES[size](w['g'])
    _tiled_launch(w, B, 13 + B, mode)


@pytest.mark.gpu
@pytest.mark.parametrize('shipped', [False, True])
def test_states_at_a_stride_beyond_nx_with_nan_in_the_padding(shipped):
    import torch
    from warm_start_hmpc_amd.qp_backend import HipBatchedQP
    c = sk.nodes(WALLS, 10)
    nx, B = 4, 40
    with _env(HMPC_JIT=0) if shipped else contextlib.nullcontext():
        qp = HipBatchedQP(c['ctrl'].problem_data())  # a fresh handle: the first call of a compiled kernel goes through hmpc_check_set_kernel
    assert qp.kernel_info() == ((2, 2, 2) if shipped else (6, 6, 6)), qp.kernel_info()
    states = np.linspace(.3, 1., B)[:, None] * c['x0'][None, :] + np.linspace(-.2, .2, B)[:, None] * np.array([0., 1., 0., 0.])
    wide = np.full((B, nx + 3), np.nan)
    wide[:, :nx] = states
    fix = _to(c['fix'][:B])
    strided = _launch(qp, _to(wide), fix, x0_stride=nx + 3)
    packed = _launch(qp, _to(states), fix)
    _assert_same_bits(strided, packed, what='x0_stride = nx + 3')
    status = packed['status'].cpu().numpy()
    assert (status == 0).sum() >= 8 and (status == 1).sum() >= 8 and np.all(status <= 1), np.bincount(status)
    one = _launch(qp, _to(states[7]), fix)           # ... and the states do matter: one shared state gives other records
    assert not torch.equal(_bits(one['obj']), _bits(packed['obj']))
    assert qp.kernel_info() == ((2, 2, 2) if shipped else (6, 6, 6)) and qp.jit_stats()[0] == 0


@pytest.mark.gpu
def test_a_stride_below_nx_is_refused():
    w = _order_workload(WALLS, 10)
    B = 8
    out = _outputs(B, w['qp'])
    with pytest.raises(RuntimeError, match=r'\(-1\)'):                     # HMPC_EINVAL
        w['qp'].solve_batch_device(_to(np.zeros((B, 3))), w['fix'][:B].contiguous(), out, x0_stride=3)
    assert int((out['status'] == INT_SENTINEL).sum()) == B                # nothing was launched
