"""CPU tests of MPCQP_OPT_ON_CHIP_32 (csrc/mpcqp_duo.hip): the flag's value in the header and in the Python layer, the unit in the
build, the conditions that the inputs of tests/test_gpu_onchip32.py (tests/onchip32_cases.py) satisfy on the C oracle, and a scan
of the unit's gfx950 assembly: no hand-written DPP arithmetic, the compiler's own DPP instructions inside the wait-state rules."""
import os
import re

import numpy as np
import pytest

import onchip32_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "mpcqp_duo.hip"


def test_flag_value_in_header_and_python():
    from qpmpc_amd import _capi

    text = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    opts = {name: int(val) for name, val in re.findall(r"#define (MPCQP_OPT_\w+) (\d+)", text)}
    assert opts["MPCQP_OPT_ON_CHIP_32"] == 16384 == _capi.OPT_ON_CHIP_32
    others = [v for k, v in opts.items() if k != "MPCQP_OPT_ON_CHIP_32"]
    assert len(others) >= 14 and all(v & 16384 == 0 for v in others)  # a bit of its own
    assert int(re.search(r"#define MPCQP_ABI_VERSION (\d+)", text).group(1)) == 12  # additive


def test_unit_is_built():
    from qpmpc_amd import build

    assert UNIT in build._UNITS
    assert os.path.exists(os.path.join(ROOT, "qpmpc_amd", "csrc", UNIT))
    assert f"qpmpc_amd/csrc/{UNIT}" in build.one_line_command()


@pytest.mark.parametrize("shape,kind,why", OC.SHAPES, ids=[str(s[0]) for s in OC.SHAPES])
def test_families_on_the_oracle(shape, kind, why):
    """Per shape: every problem of the per-step families is solved by the oracle at all three tightnesses, and at least half of
    each is clear; the time-invariant families may hold inconsistent problems (see onchip32_cases) but at least fifteen solved
    ones each; some solved item of the shape took a partial step or drop on the oracle (iterations above its positive
    multipliers); inside the kernel's envelope."""
    nx, nu, N, mk = shape
    assert 17 <= N * nu <= 32 and N * mk <= 64 and 1 <= mk <= 4 and 2 <= nx <= 4
    dropped = 0
    for tight in OC.TIGHT:
        for lti in (False, True):
            U, lam, st, it = OC.reference(shape, kind, tight, lti)
            ok = st == 0
            clear = OC.clear(shape, kind, tight, lti)
            print(f"    {shape} {kind} tight {tight} lti {lti}: solved {int(ok.sum())}, clear {int(clear.sum())}, "
                  f"binding {int(((lam > 0).any(axis=1) & ok).sum())}, drops {OC.drops(lam, it, ok)}")
            assert set(np.unique(st)) <= {0, 2}
            if not lti:
                assert ok.all()
                assert 2 * clear.sum() >= OC.BATCH
            else:
                assert ok.sum() >= 15 and clear.sum() >= 10
            dropped += OC.drops(lam, it, ok)
    assert dropped > 0


def test_layout_cases_on_the_oracle():
    """The operand-layout cases of the GPU test (seed 1000 + i, margin 0.2): the oracle solves all nine problems of every layout,
    at least six with a binding row."""
    import operand_layouts as OL

    for i in range(len(OL.LAYOUTS)):
        U, lam, st = OC.layout_reference(i)
        assert (st == 0).all(), (i, st)
        assert ((lam > 1e-9).any(axis=1)).sum() >= 6, i


def test_verdict_cases_on_the_oracle():
    """The verdict inputs of the GPU test: nine general problems of (3, 1, 24, 2) and of (4, 2, 16, 2) (layout 0, seed 1000,
    margin 0.2), all solved by the oracle; verdict_cases.mixed makes items 1, 6 and 7 infeasible and leaves the others solved."""
    import oracle
    import operand_layouts as OL
    import verdict_cases as VC

    for shape in ((3, 1, 24, 2), (4, 2, 16, 2)):
        full = OL.make(shape, "cd", True, 0, OC.LAYOUT_SEED, OC.LAYOUT_MARGIN)[1]
        assert (oracle.solve_workload(full)[2] == 0).all()
        st = oracle.solve_workload(VC.mixed(full)[0])[2]
        assert np.array_equal(st == 0, VC.MIXED_STATUS == 0), st


def test_assembly_carries_no_hand_written_dpp_arithmetic():
    """The unit exchanges values through what the compiler schedules itself (DPP moves, v_permlane16_swap, ds_bpermute, LDS):
    no v_fmac_f64_dpp, no inline assembly in the source, and the DPP instructions the compiler emitted keep the wait states."""
    import dpp_instantiations as DI
    import tools.check_dpp_hazards as chk

    src = open(os.path.join(ROOT, "qpmpc_amd", "csrc", UNIT)).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "asm" not in code and "fmac_bcast" not in code and "dpp_ready" not in code
    asm = DI.unit_asm(UNIT)
    assert asm.count("mpcqp_duo_kernel") >= 3
    assert "v_fmac_f64_dpp" not in asm
    bad, ndpp, nasm = chk.check(asm)
    assert ndpp > 0 and nasm == 0
    assert bad == [], [chk.describe(h) for h in bad[:5]]


def test_resources_are_recorded():
    """profiles/onchip32.md records the register, scratch and LDS figures of the three instantiations."""
    text = open(os.path.join(ROOT, "profiles", "onchip32.md")).read()
    for nx in (2, 3, 4):
        assert f"mpcqp_duo_kernel<{nx}>" in text
    assert "scratch" in text and "MPCQP_OPT_ON_CHIP_32" in text
