"""GPU tests (-m gpu): one launch per kernel that carries hand-written DPP instructions (fmac_bcast of csrc/mpcqp_lane.h: a
v_fmac_f64_dpp in inline assembly, whose wait states the source keeps with dpp_ready). What the register allocator puts between the two
differs per template instantiation -- nx = 5, 6 with four rows per lane once shipped plans that were 1e-6 .. 3 off, statuses mostly
right, no fault --, so every instantiation is launched here, by the recipe tests/dpp_instantiations.py::MANIFEST gives for it (the
smallest launch that selects it), and held to a reference: a kernel trace of this file alone shows every one of them called
(profiles/dpp_instantiations.txt).

Every bound is one an older test of the same launch shape holds:
  oracle   plans within 1e-7 max(1, |u_ref|_inf) of the C oracle, statuses equal (tests/test_gpu_quad.py)
  slim     launches of several rounds (the slim LDS carve): statuses and iteration counts bit for bit those of the same problems in two
           launches of the roomy carve, plans within 1e-9 relative; the oracle on the first 256 and the last 64 problems -- the last
           wavefront is ragged -- as above (tests/test_gpu_quad.py::test_launches_of_several_rounds_take_the_slim_carve)
  order    a pairing order made from the cold launch's iteration counts: statuses and counts equal to the natural order's, plans
           within 1e-8 (tests/test_gpu_pairing.py); the oracle as above
  two      the pair kernel in workgroups of two wavefronts: bit for bit the single-wavefront launches of the same problems,
           multipliers included; the oracle within 1e-8
           (tests/test_gpu_parity.py::test_exactly_full_launch_of_the_pair_kernel_equals_the_other_launch_shapes)
  seeded   MPCQP_OPT_SEED_VIOLATED and MPCQP_WARM_ACTIVE_SET after a cold launch that filled the state: statuses equal, plans within 1e-8 of
           the cold ones and of the oracle (tests/test_gpu_warm_start.py)
  warm     MPCQP_WARM_OPERATOR after the cold launch: statuses equal, plans within 1e-9 of the cold ones, 1e-8 of the oracle (same)
The inputs are held to their conditions (binding rows, drops, all solved) by tests/test_dpp_instantiations_cpu.py."""

import numpy as np
import pytest

import dpp_instantiations as DI

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _simds():
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def _scale(U):
    return np.maximum(1.0, np.abs(U).max(axis=1, keepdims=True))


class _Launcher:
    """the launches of one recipe: solve_mpc_batch, or one SharedModel factored from the whole family and prepared per launch"""

    def __init__(self, name, w):
        from qpmpc_amd import SharedModel, _capi
        from qpmpc_amd import workloads as W

        self.recipe = DI.MANIFEST[name]
        self.flags = 0
        for f in self.recipe["flags"]:
            self.flags |= getattr(_capi, f)
        self.model = SharedModel(W.to_batch_problem(w)) if self.recipe["entry"] == "model" else None

    def __call__(self, w, flags=None, **kw):
        from qpmpc_amd import solve_mpc_batch
        from qpmpc_amd import workloads as W

        bp = W.to_batch_problem(w)
        flags = self.flags if flags is None else flags
        if self.model is None:
            plan = solve_mpc_batch(bp, return_multipliers=True, flags=flags, **kw)
        else:
            run = self.model.prepare(bp, return_multipliers=True, flags=flags, **kw)
            run.launch()
            plan = run.plan
            plan._keep = run
        torch.cuda.synchronize()
        return plan


def _np(plan):
    return plan.U.cpu().numpy(), plan.status.cpu().numpy(), plan.iters.cpu().numpy()


def _against_oracle(name, plan, tol, absolute=False):
    """statuses and plans of the oracle-checked problems (all of a small launch, the first 256 and the last 64 of a large one)"""
    index, Uo, _, sto, _ = DI.oracle_on(name, _simds())
    U, st, _ = _np(plan)
    U, st = U[index], st[index]
    assert np.array_equal(st == 0, sto == 0), index[(st == 0) != (sto == 0)]
    ok = sto == 0
    assert ok.any() and not np.isnan(U).any()
    err = np.abs(U[ok] - Uo[ok]) / (1.0 if absolute else _scale(Uo[ok]))
    print(f"{name}: worst error against the oracle {err.max():.2e} on {int(ok.sum())} problems (bound {tol:.0e})")
    assert err.max() <= tol, (err.max(), index[ok][err.max(axis=1).argmax()])


def _halves(w):
    """the family in two launches, the cut at an even problem (between two wavefronts' pairs)"""
    half = (w["x0"].shape[0] // 2) & ~1
    return DI.take(w, slice(0, half)), DI.take(w, slice(half, None))


def _check_oracle(name, w, launch):
    _against_oracle(name, launch(w), 1e-7)


def _check_slim(name, w, launch):
    slim = launch(w)
    parts = [launch(p) for p in _halves(w)]
    st, it, U = (torch.cat([getattr(p, k) for p in parts]) for k in ("status", "iters", "U"))
    assert torch.equal(st, slim.status) and torch.equal(it, slim.iters)
    good = st == 0
    assert int(good.sum()) > len(st) // 2
    diff = float((U[good] - slim.U[good]).abs().max())
    print(f"{name}: slim against roomy carve {diff:.2e}")
    assert diff <= 1e-9 * max(1.0, float(U[good].abs().max()))
    _against_oracle(name, slim, 1e-7)


def _check_order(name, w, launch):
    from qpmpc_amd import pairing_order

    ref = launch(w)
    order = pairing_order(ref.iters)
    torch.cuda.synchronize()
    batch = len(ref.iters)
    assert np.array_equal(np.sort(order.cpu().numpy()), np.arange(batch)) and int((order != torch.arange(batch, device="cuda")).sum()) > batch // 2
    got = launch(w, order=order)
    assert torch.equal(got.status, ref.status) and torch.equal(got.iters, ref.iters)
    ok = ref.status == 0
    scale = ref.U[ok].abs().amax(dim=1, keepdim=True).clamp(min=1.0)
    diff = float(((got.U[ok] - ref.U[ok]).abs() / scale).max())
    print(f"{name}: ordered against natural launch {diff:.2e}")
    assert diff <= 1e-8
    _against_oracle(name, got, 1e-7)


def _check_two(name, w, launch):
    exact = launch(w)
    parts = [launch(p) for p in _halves(w)]
    for k in ("status", "iters", "U", "multipliers"):
        assert torch.equal(torch.cat([getattr(p, k) for p in parts]), getattr(exact, k)), k
    _against_oracle(name, exact, 1e-8, absolute=True)


def _cold_and_state(w, launch):
    from qpmpc_amd import WarmState, _capi
    from qpmpc_amd import workloads as W

    ws = WarmState(W.to_batch_problem(w))
    cold = launch(w, flags=_capi.OPT_TWO_PER_WAVE)  # the pair kernel's cold instantiation: the plans to compare with
    filled = launch(w, warm_state=ws)  # a cold start that stores the active set and the operator
    assert torch.equal(cold.status, filled.status)
    return ws, cold


def _close_to_cold(name, what, got, cold, tol):
    (U1, st1, _), (U0, st0, _) = _np(got), _np(cold)
    assert np.array_equal(st0, st1)
    ok = st0 == 0
    diff = (np.abs(U1[ok] - U0[ok]) / _scale(U0[ok])).max()
    print(f"{name}: {what} against the cold launch {diff:.2e}")
    assert diff <= tol, (what, diff)


def _check_seeded(name, w, launch):
    from qpmpc_amd import _capi

    ws, cold = _cold_and_state(w, launch)
    seeded = launch(w, flags=_capi.OPT_SEED_VIOLATED)
    _close_to_cold(name, "seed steps", seeded, cold, 1e-8)
    _against_oracle(name, seeded, 1e-8)
    rows = launch(w, warm_state=ws, warm_start="active_set", warm_shift=0)
    _close_to_cold(name, "stored rows", rows, cold, 1e-8)
    _against_oracle(name, rows, 1e-8)


def _check_warm(name, w, launch):
    ws, cold = _cold_and_state(w, launch)
    assert int((ws.active_set >= 0).sum()) > 0  # (the record holds the active rows)
    warm = launch(w, warm_state=ws, warm_start=True)
    _close_to_cold(name, "operator warm start", warm, cold, 1e-9)
    _against_oracle(name, warm, 1e-8)
    ok = cold.status == 0
    assert int(warm.iters[ok].sum()) < int(cold.iters[ok].sum())  # (it started from the stored operator, not from the empty set)


_CHECKS = dict(oracle=_check_oracle, slim=_check_slim, order=_check_order, two=_check_two, seeded=_check_seeded, warm=_check_warm)


@pytest.mark.parametrize("name", DI.REACHABLE)
def test_every_instantiation_with_hand_written_dpp_gives_the_reference_plans(name):
    recipe = DI.MANIFEST[name]
    w = DI.family(name, _simds())
    _CHECKS[recipe["check"]](name, w, _Launcher(name, w))


def test_the_instantiations_marked_unreachable_are_refused_before_any_launch():
    """mpcqp_quad_kernel<2, true, ...> (the lean build of nx = 2 with a pairing order) is compiled, but a pairing order is taken
    only where the two-per-wavefront kernel could serve the launch, and that one has nx = 3 and 4: MPCQP_EUNSUPPORTED at every
    batch size, with and without MPCQP_OPT_FOUR_PER_WAVE."""
    from qpmpc_amd import BackendError, _capi, solve_mpc_batch
    from qpmpc_amd import workloads as W

    assert sorted(k for k, r in DI.MANIFEST.items() if r.get("unreachable")) == [
        "mpcqp_quad_kernel<2, true, 1, false, false, false>", "mpcqp_quad_kernel<2, true, 1, true, false, false>"]
    for batch in (DI.SMALL, DI.BATCHES["slim"](_simds())):
        w = DI._general_family(np.random.default_rng(1), batch, 2, 1, 16, 0.2, "c", False, 2)
        order = torch.arange(batch - 1, -1, -1, dtype=torch.int32, device="cuda")
        for flags in (0, _capi.OPT_FOUR_PER_WAVE):
            with pytest.raises(BackendError, match="-6"):
                solve_mpc_batch(W.to_batch_problem(w), flags=flags, order=order)
