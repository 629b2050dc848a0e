"""CPU tests of mpcqp_solve_batch with MPCQP_OPT_ON_CHIP_32 (csrc/mpcqp_duo.hip, its QP-given mode): the conditions that the inputs
of tests/test_gpu_onchip32_qp.py (tests/onchip32_qp_cases.py) satisfy on the C oracle, the kernel in the unit's gfx950 assembly
beside the existing four, its recorded resources, and the header's text."""
import os
import re

import numpy as np
import pytest

import onchip32_qp_cases as QC
import verdict_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "mpcqp_duo.hip"
EXISTING = ("mpcqp_duo_kernel<2, false>", "mpcqp_duo_kernel<3, false>", "mpcqp_duo_kernel<4, false>", "mpcqp_duo_kernel<0, true>")
QP_KERNEL = "mpcqp_duo_kernel<0, false>"


@pytest.mark.parametrize("size,why", QC.SIZES, ids=[str(s[0]) for s in QC.SIZES])
def test_sizes_on_the_oracle(size, why):
    """Per size: the oracle's statuses are verdict_cases.MIXED_STATUS, all six solved items are clear at 1e-6, and from n = 16 up
    some item took a partial step or drop (iterations above its positive multipliers), (17, 2) excepted; at (20, 64) the active
    set reaches n, at (32, 64) one item fills all 32 slots; inside the kernel's envelope."""
    n, m = size
    assert 1 <= n <= 32 and 1 <= m <= 64
    x, lam, st, it = QC.reference(n, m)
    clear = QC.clear(n, m)
    nact = (lam > 0).sum(axis=1)
    print(f"    {size} ({why}): status {st.tolist()}, clear {int(clear.sum())}, drops {QC.drops(n, m)}, active {nact.tolist()}, "
          f"iters {it.tolist()}")
    assert np.array_equal(st, VC.MIXED_STATUS)
    assert clear.sum() == 6 == (st == 0).sum()
    if n >= 16 and size != (17, 2):
        assert QC.drops(n, m) > 0
    if size == (20, 64):
        assert (nact[st == 0] == n).sum() >= 1
    if size == (32, 64):
        assert nact[st == 0].max() == 32


def test_indefinite_item_on_the_oracle():
    """P[5][5] -= 50 on item 3 of (24, 48): the oracle says status 3 after no iteration, and leaves the other items' verdicts"""
    import oracle

    P, q, G, h = QC.indefinite(24, 48)
    b = QC.INDEFINITE_ITEM
    _, _, st, it = oracle.gi_solve(P[b], q[b], G[b], h[b])
    assert (st, it) == (3, 0)
    assert VC.MIXED_STATUS[b] == 0


@pytest.mark.parametrize("shape", QC.MPC_SHAPES, ids=str)
def test_mpc_families_on_the_oracle(shape):
    """The MPC families of the GPU test are outside the fused flag's envelope (nx >= 5 or more than four rows per step), inside
    the QP mode's once condensed, and the oracle solves all nine of each with a binding row."""
    nx, nu, N, mk = shape
    assert (nx >= 5 or mk > 4) and 17 <= N * nu <= 32 and N * mk <= 64
    U, lam, st, it = QC.mpc_reference(shape)
    assert (st == 0).all() and (lam > 1e-9).any(axis=1).all(), (st, (lam > 1e-9).sum(axis=1))


def test_assembly_holds_the_qp_kernel_beside_the_existing_four():
    import dpp_instantiations as DI

    asm = DI.unit_asm(UNIT)
    names = {DI.demangle(s) for s in re.findall(r"^(_ZN5mpcqp\w+):", asm, flags=re.M)}
    for k in EXISTING + (QP_KERNEL,):
        assert k in names, (k, sorted(n for n in names if n))


def test_resources_are_recorded():
    """profiles/onchip32_qp.md records the kernel's registers, scratch and LDS"""
    text = open(os.path.join(ROOT, "profiles", "onchip32_qp.md")).read()
    assert QP_KERNEL in text and "MPCQP_OPT_ON_CHIP_32" in text
    for word in ("VGPR", "scratch", "LDS"):
        assert word in text, word


def test_header_keeps_the_abi_and_names_the_export_under_the_flag():
    text = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert int(re.search(r"#define MPCQP_ABI_VERSION (\d+)", text).group(1)) == 12
    flag = text[text.index("#define MPCQP_OPT_ON_CHIP_32"):text.index("/* MpcqpSolveOpts.warm_start */")]
    assert "mpcqp_solve_batch" in flag
    export = text[text.index("Replaces qpsolvers.solve_problem"):text.index("int mpcqp_solve_batch(")]
    assert "MPCQP_OPT_ON_CHIP_32" in export and "MPCQP_EUNSUPPORTED" in export
