"""GPU tests (-m gpu): the shared-model mode of csrc/mpcqp_duo.hip -- mpcqp_solve_model_bounds_batch (bounds per problem) and, with
MPCQP_OPT_ON_CHIP_32, mpcqp_solve_model_batch at 17 .. 32 variables and at most 64 rows, two problems per wavefront, the rows of M
and L^-T read from the factored model (the reference's build-once usage: MPCQP once, then update_cost_vector /
update_constraint_vector per period, qpmpc/mpc_qp.py:129-163). The inputs are those of tests/onchip32_model_cases.py, held to
their conditions on the C oracle by tests/test_onchip32_model_cpu.py.

Every launch goes through ctypes with its buffers in the guarded arena of tests/arena.py (ModelCase of tests/guarded_launch.py,
the model factored outside the arena): the factored model is a read-only buffer there, so a solve that wrote into it is named.

Tolerances (float64): plans |u - u_ref|_inf <= 1e-7 max(1, |u_ref|_inf) against the C oracle on the materialised problems
(guarded_launch.against_oracle); model against fused 1e-8 max(1, |u|_inf) (tests/test_gpu_quad.py holds its model mode
to the same); multipliers onchip32_cases.LAM_BOUND on the clear problems; the walking loop 1e-9 against the rebuilding loop and
1e-7 against the oracle loop (tests/test_gpu_parity.py); gradients model_adjoint_np.TOL."""
import os

import numpy as np
import pytest

import onchip32_cases as OC
import onchip32_model_cases as MC
import operand_layouts as OL
import verdict_cases as VC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guarded_launch as GL  # noqa: E402  (the arena launchers and comparisons; needs torch)
from guarded_launch import ModelCase, _flag  # noqa: E402

Z, F, F64, F32, I32, U8 = GL.Z, GL.F, GL.F64, GL.F32, GL.I32, GL.U8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULT_GOLDEN_VARIANT, FUSED_GOLDEN = MC.DEFAULT_GOLDEN_VARIANT, MC.FUSED_GOLDEN


_CASES = {}


def _case(shape, variant):
    if (shape, variant) not in _CASES:
        _CASES[(shape, variant)] = ModelCase(MC.case(shape, variant)[0], OL.model_pads(variant))
    return _CASES[(shape, variant)]


def _many(count):
    if ("many", count) not in _CASES:
        _CASES[("many", count)] = ModelCase(MC.many(count)[0])
    return _CASES[("many", count)]


def _same_bits(a, b, items_a, items_b, what):
    for name in ("U", "lam", "status", "iters"):
        assert GL.same_bits(a[name][items_a], b[name][items_b]), (what, name)


def default_route_outputs():
    """The export without bounds and without a flag on variant DEFAULT_GOLDEN_VARIANT of (3, 1, 24, 2): the default route of
    shared-model solves (tools/gen_golden_onchip32_parent.py stores what this returns)."""
    return _case(MC.PLAIN, DEFAULT_GOLDEN_VARIANT).run(F, 0, bounds=False)


def fused_outputs(fam):
    """(U, lam, status, iters) of the flagged fused launch on a family of onchip32_cases"""
    return GL.solve_outputs(OC.family(*fam), _flag())


# ---------------------------------------------------------------------------------------------- 1. parity and layouts
@pytest.mark.parametrize("shape,why", MC.SHAPES, ids=[str(s[0]) for s in MC.SHAPES])
def test_parity_and_layouts(shape, why):
    """Every variant of operand_layouts.MODEL_VARIANTS (x0, goal, targets, e per problem or shared; the odd ones padded): the
    bounds export without and with the flag, and the export without bounds with the flag where the variant shares e. All solved,
    plans within 1e-7 of the oracle on the materialised problems, no NaN; the flag changes no bit of the bounds export (one
    kernel serves both)."""
    for variant in MC.VARIANTS:
        case, full = _case(shape, variant), MC.case(shape, variant)[1]
        plain = case.run(F, 0, bounds=True)
        flagged = case.run(F, _flag(), bounds=True)
        launches = [("bounds", plain), ("bounds, flag", flagged)]
        if MC.shares_e(variant):
            launches.append(("model bounds, flag", case.run(F, _flag(), bounds=False)))
        for what, out in launches:
            assert (out["status"] == 0).all(), (what, variant, out["status"])
            ok = GL.against_oracle(f"model {shape} {variant}", full, out, 1e-7)
            assert ok.all() and not np.isnan(out["U"]).any() and not np.isnan(out["lam"]).any()
        _same_bits(plain, flagged, slice(None), slice(None), f"variant {variant}: flag on the bounds export")


def test_default_route_without_bounds_did_not_move():
    """mpcqp_solve_model_batch without a flag at (3, 1, 24, 2) still takes the workgroup kernel: U, lam, status and iters are bit for
    bit those of the commit before the on-chip model mode (tests/golden/onchip32_model_default_parent.npz, captured on an MI355X
    by tools/gen_golden_onchip32_parent.py)."""
    out = default_route_outputs()
    gold = np.load(os.path.join(GOLDEN, "onchip32_model_default_parent.npz"))
    assert (out["status"] == 0).all()
    for name in ("U", "lam", "status", "iters"):
        assert GL.same_bits(out[name], gold[name]), name


# ---------------------------------------------------------------------------------------------- 2. memory discipline
@pytest.mark.parametrize("batch", [1, 5, MC.MANY])
def test_memory_discipline(batch):
    """Bounds per problem, 1, 5 and 61 problems of (3, 1, 24, 2) (an idle half; several wavefronts with an idle half): guards
    intact, operands and model unchanged (ModelCase.run), outputs bit-equal run to run and under the 0x00 and 0xFF fills, nothing
    written next to lam and iters when they are NULL, plans within 1e-7 of the oracle."""
    case = _many(batch)
    z1, z2, f = case.run(Z), case.run(Z), case.run(F)
    GL.equal_outputs(z1, z2, f"batch {batch}: run to run under fill Z")
    GL.equal_outputs(z1, f, f"batch {batch}: fill Z against fill F")
    nn = case.run(F, lam=False, iters=False)
    assert GL.holds(nn["lam"], F) and GL.holds(nn["iters"], F), "a NULL output's neighbour was written"
    GL.equal_outputs(f, nn, f"batch {batch}: lam and iters NULL", lam=False, iters=False)
    Uo, _, sto, _ = MC.many_reference(batch)
    assert (sto == 0).all() and (f["status"] == 0).all(), (f["status"], sto)
    err = float((np.abs(f["U"] - Uo) / np.maximum(1.0, np.abs(Uo).max(axis=1, keepdims=True))).max())
    print(f"    batch {batch}: max rel err vs oracle {err:.2e}, iters mean {f['iters'].mean():.1f}")
    assert err <= 1e-7 and not np.isnan(f["U"]).any()


# ---------------------------------------------------------------------------------------------- 3. neighbours, batch size
def test_neighbour_and_batch_independence_bit_for_bit():
    """61 problems of (3, 1, 24, 2) with bounds per problem, the same in reverse order (every problem meets another neighbour and
    the other half of its wavefront), and the first 1, 2 and 3 alone: status, iters, U and lam of every item have the same bits in
    every launch."""
    w = MC.many(MC.MANY)[0]
    ref = _many(MC.MANY).run(F)
    assert (ref["status"] == 0).all()
    idx = np.arange(MC.MANY)
    rev = ModelCase(MC.take(w, idx[::-1])).run(F)
    _same_bits(ref, rev, idx, idx[::-1], "reversed")
    for count in (1, 2, 3):
        part = ModelCase(MC.take(w, idx[:count])).run(F)
        _same_bits(ref, part, idx[:count], idx[:count], f"first {count}")


# ---------------------------------------------------------------------------------------------- 4. verdicts
@pytest.mark.parametrize("shape", MC.VERDICT_SHAPES, ids=str)
def test_verdicts(shape):
    """verdict_cases.model_mixed (items 1, 6, 7 infeasible: status 2, U and lam zero; the others solved with the bits of a launch of
    the good items' own problems next to other neighbours), a model factored from a terminal weight of -50 (status 3 for all,
    iters 0, U zero), and an iteration limit chosen from the clean launch's own counts (items below it keep their bits, items
    above it: status 1, U zero, iters <= the limit)."""
    wm, _, _ = VC.model_mixed(shape)
    mixed = ModelCase(wm).run(F)
    assert np.array_equal(mixed["status"], VC.MIXED_STATUS), mixed["status"]
    bad, good = list(VC.INFEASIBLE), np.array(VC.GOOD)
    assert (mixed["U"][bad] == 0).all() and (mixed["lam"][bad] == 0).all()
    # the clean launch: the same model and the good items alone (other neighbours, another batch size)
    clean = ModelCase(MC.take(wm, good)).run(F)
    assert (clean["status"] == 0).all()
    _same_bits(mixed, clean, good, np.arange(len(good)), "solvable items next to infeasible ones")
    # not positive definite: the verdict comes with the model
    ind = ModelCase(MC.case(shape, 0)[0], wt=VC.W_TERMINAL_INDEFINITE).run(F)
    assert (ind["status"] == 3).all() and (ind["iters"] == 0).all() and (ind["U"] == 0).all()
    # iteration limit
    case = _case(shape, 0)
    full = case.run(F)
    assert (full["status"] == 0).all()
    k, below, above = VC.choose_limit(full["iters"])
    assert k is not None and below >= 2 and above >= 2, full["iters"]
    lim = case.run(F, max_iter=int(k))
    lo, hi = np.flatnonzero(full["iters"] <= k - 1), np.flatnonzero(full["iters"] >= k + 1)
    _same_bits(full, lim, lo, lo, "below the limit")
    assert (lim["status"][hi] == 1).all() and (lim["U"][hi] == 0).all() and (lim["iters"][hi] <= k).all(), (lim["status"], lim["iters"])


# ---------------------------------------------------------------------------------------------- 5. model against fused
@pytest.mark.parametrize("shape", MC.VERDICT_SHAPES, ids=str)
def test_model_against_fused(shape):
    """Variant 0: the model launch and solve_mpc_batch(flags=OPT_ON_CHIP_32) on the materialised problems give equal statuses,
    plans within 1e-8 max(1, |u|_inf) and, on the clear problems (onchip32_cases.clear's rule), multipliers within
    onchip32_cases.LAM_BOUND of each other and of the oracle."""
    from qpmpc_amd import solve_mpc_batch
    from qpmpc_amd import workloads as W

    full = MC.case(shape, 0)[1]
    out = _case(shape, 0).run(F)
    plan = solve_mpc_batch(W.to_batch_problem(full), flags=_flag(), return_multipliers=True)
    torch.cuda.synchronize()
    Uf, lamf, stf = plan.U.cpu().numpy(), plan.multipliers.cpu().numpy(), plan.status.cpu().numpy()
    assert np.array_equal(out["status"], stf) and (stf == 0).all(), (out["status"], stf)
    err = float((np.abs(out["U"] - Uf) / np.maximum(1.0, np.abs(Uf).max(axis=1, keepdims=True))).max())
    Uo, lamo, sto, _ = MC.reference(shape, 0)
    clear = MC.clear(full, Uo, lamo, sto)
    assert clear.sum() >= 3, clear
    scale = 1.0 + lamo[clear].max(axis=1, keepdims=True)
    dev_f = float((np.abs(out["lam"][clear] - lamf[clear]) / scale).max())
    dev_o = float((np.abs(out["lam"][clear] - lamo[clear]) / scale).max())
    print(f"    {shape}: model vs fused plan {err:.2e}; multipliers on {int(clear.sum())} clear items: vs fused {dev_f:.2e}, vs oracle {dev_o:.2e}")
    assert err <= 1e-8
    assert np.array_equal(out["lam"][clear] > 0, lamo[clear] > 0)
    assert dev_f <= OC.LAM_BOUND and dev_o <= OC.LAM_BOUND


# ---------------------------------------------------------------------------------------------- 6. the walking loop
def test_walking_loop_on_the_shared_model():
    """LIPMWalkingLoop at nb_timesteps = 32, sampling_period = 0.05 (the reference's walking controller sampled twice as fine over
    the same 1.6 s horizon) with shared_model=True: it constructs and runs 40 periods without a failed solve; the states equal
    those of the rebuilding loop with flags=OPT_ON_CHIP_32 to 1e-9 over the episode, and eight walkers stay within 1e-7 of the
    oracle loop (oracle/lipm_np.py with the C oracle as its solver)."""
    import oracle
    from qpmpc_amd.closed_loop import LIPMWalkingLoop

    kw, setting = MC.walk_kwargs(), dict(nb_timesteps=MC.WALK["nb_timesteps"], sampling_period=MC.WALK["sampling_period"])
    W, periods = MC.WALK["walkers"], MC.WALK["periods"]
    a = LIPMWalkingLoop(W, shared_model=True, **setting, **kw)
    b = LIPMWalkingLoop(W, flags=_flag(), **setting, **kw)
    Xa, worst = [a.states.cpu().numpy().copy()], 0.0
    for _ in range(periods):
        a.step()
        b.step()
        Xa.append(a.states.cpu().numpy().copy())
        worst = max(worst, (a.states - b.states).abs().max().item())
    Xa = np.stack(Xa, axis=1)
    assert a.stats()["failed"] == 0 and b.stats()["failed"] == 0, (a.stats(), b.stats())
    print(f"    shared model against the rebuilding loop over {periods} periods: {worst:.2e}")
    assert worst <= 1e-9

    def solve(problem):
        U, s, _ = oracle.solve_mpc_like_reference(problem)
        return None if s != 0 else U[:, 0]

    for i in range(MC.WALK["compared"]):
        Xo, _, So = MC.oracle_walk(i, solve)
        assert (So == 0).all()
        dev = float(np.abs(Xa[i] - Xo).max())
        assert dev <= 1e-7, (i, dev)


# ---------------------------------------------------------------------------------------------- 7. fused mode unchanged
@pytest.mark.parametrize("fam", FUSED_GOLDEN, ids=[str(f[0]) for f in FUSED_GOLDEN])
def test_fused_mode_bit_for_bit_the_parent(fam):
    """The flagged fused launch on two families of onchip32_cases: U, lam, status and iters bit for bit those of the commit before
    the kernel got its MODEL parameter (tests/golden/onchip32_fused_parent.npz, tools/gen_golden_onchip32_parent.py)."""
    gold = np.load(os.path.join(GOLDEN, "onchip32_fused_parent.npz"))
    tag = "x".join(str(v) for v in fam[0])
    for name, got in zip(("U", "lam", "status", "iters"), fused_outputs(fam)):
        assert GL.same_bits(got, gold[f"{name}_{tag}"]), (fam, name)


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    """MPCQP_EUNSUPPORTED, nothing written: the flag on models of n = 16, n = 33 and m = 65, on a float32 model, next to each of
    the other kernel choices, with an order, with a warm state; bounds per problem at n = 33 and next to the other kernel choices;
    SharedModel.solve_diff with bounds per problem at n = 40 raises before anything is launched."""
    from qpmpc_amd import SharedModel, _capi
    from qpmpc_amd import workloads as W
    from qpmpc_amd.exceptions import BackendError

    for shape in ((3, 1, 16, 2), (3, 1, 33, 1), (3, 2, 13, 5)):  # n = 16 ; n = 33 ; n = 26, m = 65
        ModelCase(MC.case(shape, 3)[0]).refused(_flag(), bounds=False)
    big = ModelCase(MC.case((3, 1, 33, 1), 0)[0])
    big.refused(0, bounds=True)
    big.refused(_flag(), bounds=True)
    ModelCase(MC.case((3, 2, 13, 5), 0)[0]).refused(0, bounds=True)
    w3, w0 = MC.case(MC.PLAIN, 3)[0], MC.case(MC.PLAIN, 0)[0]
    ModelCase(OL.f32_view(w3), dtype=F32).refused(_flag(), bounds=False)
    ModelCase(OL.f32_view(w0), dtype=F32).refused(0, bounds=True)
    shared, own = _case(MC.PLAIN, 3), _case(MC.PLAIN, 0)
    for extra in (_capi.OPT_FORCE_LDS, _capi.OPT_ONE_PER_WAVE, _capi.OPT_TWO_PER_WAVE, _capi.OPT_FOUR_PER_WAVE, _capi.OPT_SEED_VIOLATED):
        shared.refused(_flag() | extra, bounds=False)
        own.refused(extra, bounds=True)
        own.refused(_flag() | extra, bounds=True)
    for kw in (dict(order=np.arange(OL.BATCH)), dict(warm=True)):
        ModelCase(w3, **kw).refused(_flag(), bounds=False)
        ModelCase(w0, **kw).refused(0, bounds=True)
    out = shared.run(F, _flag(), bounds=False)  # (the same call without any of them runs)
    assert (out["status"] == 0).all()
    # the Python layer: n = 40 with bounds per problem
    w40 = MC.case((3, 1, 40, 1), 0)[0]
    bp = W.to_batch_problem(w40)
    model = SharedModel(bp)
    with pytest.raises(BackendError, match="bounds of its own"):
        model.solve_diff(bp.initial_state, bp.goal_state, bp.target_states, ineq_vector=bp.e)


# ---------------------------------------------------------------------------------------------- 9. derivatives, the Python layer
def test_derivatives_and_the_python_layer():
    """SharedModel.solve_diff with bounds per problem at (3, 1, 24, 2), x0 and e requiring grad: the gradients of a fixed random
    linear functional of (U, X) agree with solve_mpc_batch_diff's on the clear items within model_adjoint_np.TOL =
    1e-8 max(1, |ref|_inf); SharedModel.solve(..., ineq_vector=e) returns the plan of prepare(problem_for(..., e=e)), and
    flags=OPT_ON_CHIP_32 reaches the launch (a model without bounds per problem solved by the flagged route equals the ctypes
    launch bit for bit)."""
    from qpmpc_amd import SharedModel, solve_mpc_batch_diff
    from qpmpc_amd import workloads as W
    from model_adjoint_np import TOL

    shape = MC.PLAIN
    nx, nu, N, mk = shape
    w, full = MC.case(shape, 0)
    bp = W.to_batch_problem(w)
    model = SharedModel(bp)
    x0 = bp.initial_state.clone().requires_grad_(True)
    e = bp.e.clone().requires_grad_(True)
    U, X, plan = model.solve_diff(x0, bp.goal_state, bp.target_states, ineq_vector=e, states=True)
    assert (plan.status == 0).all()
    g = torch.Generator(device="cpu").manual_seed(7)
    cU = torch.randn(U.shape, generator=g, dtype=torch.float64).cuda()
    cX = torch.randn(X.shape, generator=g, dtype=torch.float64).cuda()
    ((U * cU).sum() + (X * cX).sum()).backward()
    fb = W.to_batch_problem(full)
    x0r = fb.initial_state.clone().requires_grad_(True)
    er = fb.e.clone().requires_grad_(True)
    Ur, Xr, planr = solve_mpc_batch_diff(fb, initial_state=x0r, ineq_vector=er, states=True)
    ((Ur * cU).sum() + (Xr * cX).sum()).backward()
    torch.cuda.synchronize()
    Uo, lamo, sto, _ = MC.reference(shape, 0)
    clear = MC.clear(full, Uo, lamo, sto)
    assert clear.sum() >= 3
    for what, got, ref in (("x0", x0.grad, x0r.grad), ("e", e.grad, er.grad)):
        got, ref = got.cpu().numpy().reshape(OL.BATCH, -1)[clear], ref.cpu().numpy().reshape(OL.BATCH, -1)[clear]
        assert np.abs(ref).max() > 1e-6
        dev = float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))
        print(f"    gradient with respect to {what}: {dev:.2e}")
        assert dev <= TOL, (what, dev)
    # solve(ineq_vector=) is prepare(problem_for(e=))
    a = model.solve(bp.initial_state, bp.goal_state, bp.target_states, return_multipliers=True, ineq_vector=bp.e)
    run = model.prepare(model.problem_for(bp.initial_state, bp.goal_state, bp.target_states, e=bp.e), return_multipliers=True)
    run.launch()
    torch.cuda.synchronize()
    assert torch.equal(a.U, run.U) and torch.equal(a.status, run.status) and torch.equal(a.multipliers, run.lam)
    assert (a.status == 0).all()
    # flags= reaches the launch: the model's own bounds, flagged, against the ctypes launch of the same problems
    w3 = MC.case(shape, 3)[0]
    bp3 = W.to_batch_problem(w3)
    m3 = SharedModel(bp3)
    flagged = m3.solve(bp3.initial_state, bp3.goal_state, bp3.target_states, return_multipliers=True, flags=_flag())
    torch.cuda.synchronize()
    out = _case(shape, 3).run(F, _flag(), bounds=False)
    assert GL.same_bits(flagged.U.cpu().numpy(), out["U"]) and np.array_equal(flagged.iters.cpu().numpy(), out["iters"])
    from qpmpc_amd import _capi
    from qpmpc_amd.exceptions import BackendError

    with pytest.raises(BackendError):  # (and a launch the flag cannot serve is refused, not sent elsewhere)
        m3.solve(bp3.initial_state, bp3.goal_state, bp3.target_states, flags=_flag() | _capi.OPT_FORCE_LDS)
