"""CPU tests of the shared-model mode of csrc/mpcqp_duo.hip: the conditions that the inputs of tests/test_gpu_onchip32_model.py
(tests/onchip32_model_cases.py) satisfy on the C oracle, the declarations and the documents of the mode, and the goldens its GPU
tests compare against. The scan of the unit's assembly (no hand-written DPP arithmetic, wait states) is
tests/test_onchip32_cpu.py's: it compiles the whole unit, the new instantiation included."""
import os
import re

import numpy as np
import pytest

import onchip32_model_cases as MC
import operand_layouts as OL
import verdict_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape,why", MC.SHAPES, ids=[str(s[0]) for s in MC.SHAPES])
def test_cases_on_the_oracle(shape, why):
    """Per shape, inside the mode's envelope (17 <= n <= 32, 1 <= m <= 64): the oracle solves all nine problems of every variant,
    and some solved item of the shape took a partial step or drop (iterations above its positive multipliers)."""
    nx, nu, N, mk = shape
    assert 17 <= N * nu <= 32 and 1 <= N * mk <= 64
    dropped = 0
    for variant in MC.VARIANTS:
        w, full = MC.case(shape, variant)
        assert w["A"].shape[0] == w["B"].shape[0] == w["C"].shape[0] == w["D"].shape[0] == 1  # a shared model
        U, lam, st, it = MC.reference(shape, variant)
        assert (st == 0).all(), (variant, st)
        d = MC.drops(lam, it, st == 0)
        print(f"    {shape} variant {variant}: binding {int((lam > 0).any(axis=1).sum())}, drops {d}")
        dropped += d
    assert dropped > 0


def test_shapes_cover_what_the_fused_build_cannot():
    from qpmpc_amd.workloads import random_ltv  # noqa: F401  (the cases are drawn by it)

    shapes = [s for s, _ in MC.SHAPES]
    assert any(mk > 4 for _, _, _, mk in shapes) and any(nx > 4 for nx, _, _, _ in shapes)
    assert any(N * nu == 17 for _, nu, N, _ in shapes) and any(N * nu == 32 and N * mk == 64 for _, nu, N, mk in shapes)
    assert any(N * mk <= 32 for _, _, N, mk in shapes) and any(N * mk == 63 for _, _, N, mk in shapes)


def test_many_problems_on_the_oracle():
    """The 61 problems of the batch-size tests: all solved, most with a binding row, some with a partial step; the first problems
    of the smaller batches are the first of the large one."""
    U, lam, st, it = MC.many_reference(MC.MANY)
    assert (st == 0).all()
    assert ((lam > 1e-9).any(axis=1)).sum() * 2 >= MC.MANY and MC.drops(lam, it, st == 0) > 0
    for count in (1, 5):
        assert np.array_equal(MC.many(count)[0]["e"], MC.many(MC.MANY)[0]["e"][:count])
        assert np.array_equal(MC.many_reference(count)[0], U[:count])


@pytest.mark.parametrize("shape", MC.VERDICT_SHAPES, ids=str)
def test_verdict_cases_on_the_oracle(shape):
    """verdict_cases.model_mixed: status VC.MIXED_STATUS on the oracle; the clean problems (variant 0) are all solved, their
    iteration counts leave a limit with two items on either side, and at least three of them are clear."""
    import oracle

    _, full, _ = VC.model_mixed(shape)
    assert np.array_equal(oracle.solve_workload(full)[2], VC.MIXED_STATUS)
    U, lam, st, it = MC.reference(shape, 0)
    assert (st == 0).all()
    k, below, above = VC.choose_limit(it)
    assert k is not None and below >= 2 and above >= 2
    assert MC.clear(MC.case(shape, 0)[1], U, lam, st).sum() >= 3


def test_walking_loop_inputs_on_the_oracle():
    """The walkers the GPU test compares with the oracle loop: 40 periods at nb_timesteps = 32, sampling_period = 0.05 without a
    failed solve (the seed is held here: a state on its ZMP bound makes the loop sensitive to 1e-10 of noise on the input)."""
    import oracle

    def solve(problem):
        U, s, _ = oracle.solve_mpc_like_reference(problem)
        return None if s != 0 else U[:, 0]

    assert len(MC.walk_kwargs()["index"]) == MC.WALK["walkers"]
    for i in range(MC.WALK["compared"]):
        X, _, S = MC.oracle_walk(i, solve)
        assert (S == 0).all(), (i, S)
        assert X.shape == (MC.WALK["periods"] + 1, 3) and np.isfinite(X).all()


def test_declarations_and_documents():
    """duo_model_applies / launch_duo_model are declared in mpcqp_internal.h; include/mpcqp.h documents the flag at both model
    exports; the ABI version did not move (an additive part); the mode's resource figures are recorded."""
    internal = open(os.path.join(ROOT, "qpmpc_amd", "csrc", "mpcqp_internal.h")).read()
    assert "bool duo_model_applies(const KernelArgs &ka);" in internal
    assert "int launch_duo_model(const KernelArgs &ka, int64_t batch, hipStream_t st);" in internal
    header = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert int(re.search(r"#define MPCQP_ABI_VERSION (\d+)", header).group(1)) == 12
    for export in ("mpcqp_solve_model_batch", "mpcqp_solve_model_bounds_batch"):
        decl = header.index(f"int {export}(")
        comment = header[header.rindex("\n\n", 0, decl):decl]
        assert "MPCQP_OPT_ON_CHIP_32" in comment, export
    at = header.index("#define MPCQP_OPT_ON_CHIP_32")
    flag = header[at:header.index("*/", at)]  # (the comment that follows the value)
    assert "mpcqp_solve_model_bounds_batch" in flag and "mpcqp_solve_model_batch" in flag and "only:" not in flag.split("\n")[0]
    prof = open(os.path.join(ROOT, "profiles", "onchip32_model.md")).read()
    assert "mpcqp_duo_kernel<0, true>" in prof and "scratch" in prof
    for nx in (2, 3, 4):
        assert f"mpcqp_duo_kernel<{nx}, false>" in prof and f"mpcqp_duo_kernel<{nx}>" in prof


def test_goldens_are_data():
    """The two goldens of the GPU tests: arrays of the expected shapes and types, nothing else."""
    import onchip32_cases as OC

    g = np.load(os.path.join(ROOT, "tests", "golden", "onchip32_model_default_parent.npz"), allow_pickle=False)
    assert sorted(g.files) == ["U", "iters", "lam", "status"]
    assert g["U"].shape == (OL.BATCH, 24) and g["lam"].shape == (OL.BATCH, 48) and (g["status"] == 0).all()
    f = np.load(os.path.join(ROOT, "tests", "golden", "onchip32_fused_parent.npz"), allow_pickle=False)
    for tag, n, m in (("3x1x24x2", 24, 48), ("4x2x16x2", 32, 32)):
        assert f[f"U_{tag}"].shape == (OC.BATCH, n) and f[f"lam_{tag}"].shape == (OC.BATCH, m)
        assert f[f"status_{tag}"].dtype == np.int32 and f[f"iters_{tag}"].dtype == np.int32
