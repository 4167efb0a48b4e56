"""Writes tests/golden/narrow_stage_parent.npz: the records of the nodes of tests/narrow_stage_cases.py as the kernels of THIS
checkout return them -- run on a checkout of the commit before the narrow stage body of factor_reg (a GPU box), with this script
and tests/narrow_stage_cases.py copied into it:

    python tests/golden/make_narrow_stage_parent.py [output.npz]

Per problem, wave count (1 / 2 / 4) and instantiation: obj, dual_obj, status, iters, primal, dual of every node for the cold
kernel; for the hand-down instantiation the rows that differ from the cold kernel's (``rows``: their indices -- a node that is
handed nothing takes the cold path, which equals the cold kernel to the bit).  tests/test_gpu_narrow_stage.py compares at 1e-12.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: F401,E402  (puts the package on the path)
import numpy as np  # noqa: E402
from narrow_stage_cases import cases, kernel_records, FIELDS  # noqa: E402


def raw(rec):
    """The six arrays as hmpc_solve_batch writes them (the flags back in ``iters``)."""
    out = {k: rec[k] for k in FIELDS}
    out['iters'] = rec['iters'] | (rec['polished'] << 16) | (rec['weak'] << 17) | (rec['handed'] << 18) | (rec['second'] << 19) | (rec['uncertified'] << 20)
    return out


if __name__ == '__main__':
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'narrow_stage_parent.npz')
    store = {}
    for name, c in cases().items():
        ctrl, qp = c['make']('hip')
        assert qp.kernel_info() == (6, 6, 6), (name, qp.kernel_info())   # (the kernels compiled for the problem: the ones the test runs)
        recs = kernel_records(qp, c['x0'], c['fix'])
        store[name + '/fix'] = c['fix']
        for (waves, kind), rec in recs.items():
            r = raw(rec)
            if kind == 'handdown':
                cold = raw(recs[(waves, 'cold')])
                differ = np.zeros(len(c['fix']), bool)
                for k in FIELDS:
                    a, b = r[k].reshape(len(differ), -1), cold[k].reshape(len(differ), -1)
                    differ |= ~((a == b) | ((a != a) & (b != b))).all(axis=1)
                rows = np.flatnonzero(differ)
                store['%s/%s/%s/rows' % (name, waves, kind)] = rows
                r = {k: v[rows] for k, v in r.items()}
            for k in FIELDS:
                store['%s/%s/%s/%s' % (name, waves, kind, k)] = r[k]
            print(name, waves, kind, 'statuses', np.bincount(rec['status']).tolist(), 'handed', int(rec['handed'].sum()), flush=True)
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print('%s: %d bytes' % (path, size))
    assert size < 1 << 20, 'a committed file stays below 1 MiB'
