"""CPU: the random problem families of qpmpc_amd/workloads.py (random_ltv, tight_ltv) are importable the two ways their users
import them, need nothing but NumPy, and draw dimensions inside the envelopes the kernels are tested on."""
import os
import subprocess
import sys

import numpy as np
import pytest

from qpmpc_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stress_stagewise_keeps_random_ltv_under_its_old_name(monkeypatch):
    """bench.py puts tools/ on the path and imports random_ltv from stress_stagewise: that name is the function of workloads.py.
    So are draw and row_residuals of stress_tight, for callers that import them from the script."""
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    before = {name: sys.modules.pop(name, None) for name in ("stress_stagewise", "stress_tight")}
    try:
        import stress_stagewise
        import stress_tight

        assert stress_stagewise.random_ltv is W.random_ltv
        assert stress_tight.draw is W.tight_ltv and stress_tight.row_residuals is W.row_residuals
    finally:
        for name, module in before.items():
            sys.modules.pop(name, None)
            if module is not None:
                sys.modules[name] = module


def test_families_run_without_torch():
    code = ("import sys; sys.modules['torch'] = None  # import torch now raises ImportError\n"
            "try:\n    import torch\nexcept ImportError:\n    pass\nelse:\n    raise SystemExit('torch imported')\n"
            "import numpy as np\n"
            "from qpmpc_amd.workloads import random_ltv, tight_ltv\n"
            "w = random_ltv(np.random.default_rng(1), 3, 3, 1, 16, 2, 0.3)\n"
            "assert w['A'].shape == (3, 16, 3, 3) and w['e'].shape == (3, 16, 2)\n"
            "for kind in ('narrow', 'wide', 'widef', 'general'):\n"
            "    assert tight_ltv(kind, np.random.default_rng(1), 2, 0.3)['x0'].shape[0] == 2\n"
            "assert sys.modules['torch'] is None\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("kind", ["narrow", "wide", "widef", "general"])
def test_tight_ltv_dimensions_stay_inside_the_kernel_envelopes(kind):
    for seed in range(12):
        w = W.tight_ltv(kind, np.random.default_rng(seed), 2, 0.3)
        nx, nu, N = w["A"].shape[-1], w["B"].shape[-1], int(w["N"])
        assert w["A"].shape == (2, N, nx, nx) and w["B"].shape == (2, N, nx, nu) and w["e"].shape[:2] == (2, N)
        if kind == "narrow":
            assert nx <= 4 and nu <= 2
        elif kind == "general":
            assert 17 <= nx <= 32 and nu <= 8
        else:
            assert 5 <= nx <= 16 and nu <= 4
        assert w["C"].shape[1] == w["D"].shape[1] == (1 if kind == "widef" else N)
