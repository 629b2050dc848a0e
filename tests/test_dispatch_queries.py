"""CPU test (no GPU): the host-only size queries answer exactly what tests/golden/dispatch_queries.npz recorded
(tools/gen_golden_dispatch.py) -- return code and value of mpcqp_workspace_bytes, mpcqp_stagewise_workspace_bytes,
mpcqp_warm_state_bytes, mpcqp_warm_state_kind, mpcqp_lds_bytes and mpcqp_solve_workspace_bytes over a grid that crosses
every branch of the launch dispatch. A difference is a change in what callers are told to allocate. Only the queries are
called: no launch entry point, so nothing here touches a device."""
import os

import numpy as np

from golden_util import GOLDEN

import tools.gen_golden_dispatch as gen

from qpmpc_amd import _capi


def _mismatches(name, got, want, dims):
    bad = np.argwhere(got != want)
    rows = sorted({int(i[0]) for i in bad})
    return [f"{name} {dims[r].tolist()}: got {got[r].tolist()}, recorded {want[r].tolist()}" for r in rows[:10]], len(rows)


def test_size_queries_match_golden():
    z = np.load(os.path.join(GOLDEN, "dispatch_queries.npz"))
    assert tuple(z["batches"]) == gen.BATCHES and tuple(z["max_active"]) == gen.MAX_ACTIVE
    lib = _capi.load()
    dims, sdims = z["dims"], z["solve_dims"]
    got = gen.query(lib, dims)
    got["solve"] = gen.query_solve(lib, sdims)
    report, total = [], 0
    for name, g in got.items():
        assert g.shape == z[name].shape, name
        lines, n = _mismatches(name, g, z[name], sdims if name == "solve" else dims)
        report += lines
        total += n
    assert total == 0, f"{total} rows differ (dims = dtype, nx, nu, N, mk, flags):\n" + "\n".join(report)
