"""CPU tests of tests/dpp_instantiations.py: the manifest of the kernels that carry hand-written DPP instructions is complete, and the
inputs of tests/test_gpu_dpp_instantiations.py can tell a wrong kernel from a right one.

The wait states in front of fmac_bcast (qpmpc_amd/csrc/mpcqp_lane.h) are the source's business, per template instantiation: a new
instantiation must not ship without a launch that reaches it, and a retired one must not linger in the list. The census is read off
the gfx950 assembly (hipcc cross-compiles without a GPU); the inputs are held to their conditions by the C oracle alone."""
import os
import re

import numpy as np
import pytest

import dpp_instantiations as DI

SIMDS = 1024  # an MI355X: 256 compute units of four SIMDs (the GPU tests read it from the device)


def test_demangled_names_are_the_traces():
    sym = "_ZN5mpcqp17mpcqp_quad_kernelILi16ELb0ELi1ELb1ELb0ELb1EEEvPKdS2_S2_S2_S2_S2_S2_PdS3_PiS4_NS_10KernelArgsEl"
    assert DI.demangle(sym) == "mpcqp_quad_kernel<16, false, 1, true, false, true>"
    sym = "_ZN5mpcqp18mpcqp_quadg_kernelILi8ELi4ELb1EEEvPKdS2_S2_S2_S2_S2_S2_PdS3_PiS4_NS_10KernelArgsEl"
    assert DI.demangle(sym) == "mpcqp_quadg_kernel<8, 4, true>"
    assert DI.demangle("_ZN5mpcqp1fILin3EEEvv") == "f<-3>" and DI.demangle("main") is None
    asm = "_ZN5mpcqp1fILi1EEEvv:\n\tv_fmac_f64_dpp v[6:7], v[0:1], v[8:9] row_newbcast:3 row_mask:0xf bank_mask:0xf\n.LBB0_1:\n" \
          "\tv_fmac_f64_dpp v[6:7], v[0:1], v[8:9] row_newbcast:3 row_mask:0xf bank_mask:0xf\n_ZN5mpcqp1gILi1EEEvv:\n\ts_endpgm\n"
    assert DI.census_of(asm) == {"f<1>": 2}


def test_every_kernel_with_hand_written_dpp_has_a_recipe_and_no_recipe_lingers():
    """The manifest's keys are the census: the kernels of the five units that hold a v_fmac_f64_dpp. At most four of them may be
    marked unreachable, each with a verbatim quote of the rule that proves it (found once in its file, inside the function named);
    every other one has a recipe with a known check and the launcher function that selects it, in whose text a line spells it."""
    census = DI.census()
    assert set(DI.MANIFEST) == set(census), (sorted(set(census) - set(DI.MANIFEST)), sorted(set(DI.MANIFEST) - set(census)))
    assert all(count > 0 for _, count in census.values())
    unreachable = [k for k, r in DI.MANIFEST.items() if r.get("unreachable")]
    assert len(unreachable) <= 4 and len(unreachable) + len(DI.REACHABLE) == len(census)
    for name, r in DI.MANIFEST.items():
        src, _, function = r["site"].partition(":")
        source = open(os.path.join(DI.ROOT, "qpmpc_amd", "csrc", src)).read()
        text = DI.function_text(source, function)
        assert text, (name, r["site"])  # the function is found in the file, once
        if r.get("unreachable"):
            assert r["why"]
            assert source.count(r["quote"]) == 1 and "\n".join(text).count(r["quote"]) == 1, (name, r["site"])
            continue
        assert r["check"] in ("oracle", "slim", "order", "two", "seeded", "warm") and r["entry"] in ("solve", "model")
        # a line of the function names the instantiation: the kernel and its template arguments, of which trailing ones may be left
        # to the templates' defaults (false; one wavefront per block)
        kernel, args = name.split("<")[0], name.split("<")[1].rstrip(">").split(", ")
        spelled = [[{"NX": args[0], "MK": args[1], "ROWS": args[1]}.get(a, a) for a in s.split(", ")]
                   for line in text for s in re.findall(kernel + r"<([^>]*)>", line)]
        assert any(s == args[: len(s)] and all(a in ("false", "1") for a in args[len(s):]) for s in spelled), (name, r["site"], spelled)


@pytest.mark.parametrize("name", DI.REACHABLE)
def test_inputs_can_tell_a_wrong_kernel_from_a_right_one(name):
    """Of the oracle-checked problems of every case (all of a small launch; the first 256 and the last 64 of a large one) at least
    two thirds have a binding row and every problem is solved (no family here is drawn with inconsistent rows); a tight family
    (tightness at or below 0.2: all of them) has a problem with a drop -- more iterations than rows that stayed: every iteration
    of the method adds a row or drops one, so iterations - active rows = 2 drops. The oracle is the only code this runs."""
    r = DI.MANIFEST[name]
    index, U, lam, status, iters = DI.oracle_on(name, SIMDS)
    batch = DI.batch_of(r, SIMDS)
    assert len(index) == min(batch, DI.ORACLE_HEAD + DI.ORACLE_TAIL) and index[-1] == batch - 1
    assert (status == 0).all(), np.flatnonzero(status)
    binding = (lam > 0).any(axis=1)
    assert binding.mean() >= 2 / 3, binding.mean()
    if r["tight"] <= 0.2:
        assert (iters > (lam > 0).sum(axis=1)).any()
    assert np.isfinite(U).all()


def test_batches_select_what_the_recipes_say():
    """The batch rules restated from the launch code: slim carves and the pair kernel's one-round window, at several device sizes."""
    for simds in (1024, 304 * 4, 64):
        slim, slim4, window = (DI.BATCHES[k](simds) for k in ("slim", "slim4", "window"))
        assert (slim + 3) // 4 > simds and slim % 4 and (slim // 2 + 3) // 4 <= simds  # (two shards take the roomy carve)
        assert (slim4 + 3) // 4 > 3 * (simds // 4) and slim4 % 4 and (slim4 // 2 + 1 + 3) // 4 <= 3 * (simds // 4)
        waves = (window + 1) // 2
        assert 2 * simds - 8 < waves <= 2 * simds and window % 2 and waves % 2
        half = window // 2  # (the comparison launches: two halves, the cut between two wavefronts, each outside the window)
        assert half % 2 == 0 and (window - half + 1) // 2 <= 2 * simds - 8
    assert (DI.SMALL + 3) // 4 <= 64 and DI.SMALL % 4 and DI.SMALL % 2
