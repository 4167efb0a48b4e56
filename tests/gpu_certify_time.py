"""Timing of the certificate kernel alone on the 4096-node N = 20 replay frontier (diagnostic, run by hand; not collected):
kernel time, bytes of the rows read, the resulting TB/s, and the solve time of the same batch beside it."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import conftest  # noqa
import numpy as np
import torch
from helpers import make_controller, load_fixture
import bench
from certify_reference import COLUMNS

B = int(os.environ.get('CERTIFY_NODES', '4096'))
ctrl = make_controller('cart_pole_with_walls', T=20, backend='hip')
qp, dev = ctrl.qp, torch.device('cuda', 0)
x0, fix, _ = bench.real_tree_frontier(ctrl, B, 0, load_fixture('cart_pole_with_walls')['x_max'], spread=0)
d_x0, d_fix = torch.tensor(x0, device=dev), torch.tensor(fix, device=dev)
out = dict(obj=torch.empty(B, dtype=torch.float64, device=dev), dual_obj=torch.empty(B, dtype=torch.float64, device=dev),
           status=torch.empty(B, dtype=torch.int32, device=dev), iters=torch.empty(B, dtype=torch.int32, device=dev),
           primal=torch.empty((B, qp.n_primal), dtype=torch.float64, device=dev), dual=torch.empty((B, qp.n_dual), dtype=torch.float64, device=dev))
res = torch.empty((B, len(COLUMNS)), dtype=torch.float64, device=dev)
verdict = torch.empty(B, dtype=torch.int32, device=dev)


def timed(call, reps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


solve_ms = timed(lambda: qp.solve_batch_device(d_x0, d_fix, out), 10)
status = out['status'].cpu().numpy()
for stage in ('2', '1', '0'):
    os.environ['HMPC_CERTIFY_STAGE'] = stage      # (a test switch read by hmpc_create: a handle of its own per form)
    cq = make_controller('cart_pole_with_walls', T=20, backend='hip').qp
    ms = timed(lambda: cq.certify_batch_device(d_x0, d_fix, out, res, verdict), 50)
    # rows read: the dual row of every decided record, the primal row of every one (values of an optimal record, the NaN count of a ray)
    nbytes = 8 * int((status <= 1).sum()) * (qp.n_primal + qp.n_dual)
    v = verdict.cpu().numpy()
    print('certify: %d nodes (%d optimal, %d infeasible, %d failed), HMPC_CERTIFY_STAGE=%s: %.4f ms, %.1f MB of rows, %.3f TB/s; solve of the same batch %.3f ms, ratio %.4f'
          % (B, (status == 0).sum(), (status == 1).sum(), ((v & 0x100) != 0).sum(), stage, ms, nbytes / 1e6, nbytes / ms / 1e9, solve_ms, ms / solve_ms), flush=True)
