"""GPU tests (-m gpu): the memory contract of include/mpcqp.h, export by export. Every pointer of a call is caller-owned, the
*_workspace_bytes queries name what a launch needs, the workspace's initial content is never read (outside the documented
KEEP / REUSE / PIPELINE_FACTOR and warm-start sequences) and idle rows store nothing.

Every operand, output, workspace, warm-state and model buffer of a call is carved from one guarded arena (tests/arena.py): exact
sizes, 512-byte aligned, 64 KiB of guard on either side. Each launch runs under fill Z (guards, outputs and scratch 0x00) and fill F
(0xFF: NaN in both float widths, -1 as an int32) and must

  (a) leave every guard intact,
  (b) give bit-equal outputs run to run and fill to fill, for every item whose output the header defines,
  (c) leave read-only operands, unselected items, row padding and the buffers behind NULL-ed outputs alone,
  (d) be right: forward plans against the C oracle (solved / unsolved equal, |u - u_ref| <= 1e-7 max(1, |u_ref|) in float64, 1e-3
      in float32, as tests/test_gpu_quad.py and tests/test_gpu_stress.py), condensed matrices against oracle/condense_np.py at
      1e-12 relative (tests/test_gpu_parity.py::test_mpcqp_matches_reference_fixture), derivatives against the NumPy restatements
      of tests/*_np.py at 1e-8 max(1, |ref|),
  (e) take workspace = NULL, workspace_bytes = 0 wherever the size query answers 0.

The exports are called through ctypes directly, by the launchers of tests/guarded_launch.py (Launch, Forward, discipline, ModelCase,
QPs, PlanVjp, PlanJvp). No launch ever gets a buffer smaller than the contract says."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle

import adjoint_np as AN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from guarded_launch import (F, F32, F64, I32, U8, Z, Forward, Launch, PlanJvp, PlanVjp, QPs, ModelCase, _api, _dense_qps,  # noqa: E402
                            _rel, _tangents, add_problem, against_oracle, arena_problem, close, condense_refs, discipline,
                            equal_outputs, f32_view, forward_on_cpu, holds, ltv, same_bits, same_plans)

HERE = os.path.dirname(os.path.abspath(__file__))



def test_quad_lean_four_per_wavefront():
    """mpcqp_quad.hip, lean build: BASELINE config 1's triple integrator (3, 1, 16, 2); 1 and 5 problems leave rows of the only
    wavefront idle, 61 leaves three rows of the last one idle."""
    from qpmpc_amd import _capi
    from qpmpc_amd import workloads as W

    for batch in (1, 5, 61):
        case, _ = discipline(f"quad lean {batch}", W.triple_integrator_batch(batch, seed=batch), flags=_capi.OPT_FOUR_PER_WAVE)
        # (e): the on-chip kernels need no workspace; the query says 0 and the launches above ran with workspace = NULL
        assert case.ws_bytes == 0 and case.L.ptr("ws") is None


@pytest.mark.parametrize("shape", [(6, 2, 8, 2, "cd", True), (12, 4, 4, 2, "c", False)])
def test_quad_general_registers_and_streamed(shape):
    """mpcqp_quad.hip, general build: operands in registers (nx = 6, C and D rows, a stage cost) and streamed per step (nx = 12)."""
    from qpmpc_amd import _capi

    nx, nu, N, mk, rows, stage = shape
    w = ltv(600 + nx, 5, nx, nu, N, mk, 0.2, rows, stage)
    case, forced = discipline(f"quad general {shape}", w, flags=_capi.OPT_FOUR_PER_WAVE)
    equal_outputs(forced, case.run(F, 0), "the default dispatch takes this kernel")


@pytest.mark.parametrize("shape", [(3, 1, 16, 4), (8, 4, 4, 8)])
def test_quadg_four_rows_per_lane(shape):
    """mpcqp_quadg.hip (33 .. 64 rows, or five to eight rows per step): 5 and 45 problems."""
    from qpmpc_amd import _capi

    for batch in (5, 45):
        w = ltv(700 + shape[0] + batch, batch, *shape, tight=0.2)
        case, forced = discipline(f"quadg {shape} {batch}", w, flags=_capi.OPT_FOUR_PER_WAVE)
        equal_outputs(forced, case.run(F, 0), "the default dispatch takes this kernel")


def test_pair_two_per_wavefront_and_an_order_that_leaves_one_out():
    """mpcqp_pair.hip: 3 problems leave half a wavefront idle, 61 half of the last one. Then a pairing order that names problem 7
    twice and leaves problem 11 out: "one left out keeps its old outputs"."""
    from qpmpc_amd import _capi
    from qpmpc_amd import workloads as W

    for batch in (3, 61):
        w = W.triple_integrator_batch(batch, seed=batch)
        case, two = discipline(f"pair {batch}", w, flags=_capi.OPT_TWO_PER_WAVE)
    equal_outputs(two, case.run(F, 0), "the default dispatch of 61 lean problems is the pair kernel")
    order = np.arange(61)[::-1].copy()
    order[order == 11] = 7
    case = Forward(w, order=order)
    rest = np.ones(61, dtype=bool)
    rest[11] = False
    z, f = case.run(Z), case.run(F)
    equal_outputs(z, f, "pair with an order: fill Z against fill F", items=rest)
    for out, byte in ((z, Z), (f, F)):
        for name in ("U", "lam", "status", "iters"):
            assert holds(out[name][11], byte), (name, "of the item the order leaves out was written")
    # (the two halves of a wavefront sum in different orders: plans equal to rounding, statuses and iterations equal)
    assert np.array_equal(f["status"][rest], two["status"][rest]) and np.array_equal(f["iters"][rest], two["iters"][rest])
    assert np.abs(f["U"][rest] - two["U"][rest]).max() <= 1e-9 * max(1.0, np.abs(two["U"]).max())


def test_one_per_wavefront():
    """mpcqp_w64.hip (MPCQP_OPT_ONE_PER_WAVE), (4, 2, 8, 3): one problem, and 65 (one problem on a second workgroup)."""
    from qpmpc_amd import _capi

    for batch in (1, 65):
        discipline(f"one per wavefront {batch}", ltv(800 + batch, batch, 4, 2, 8, 3, 0.3), flags=_capi.OPT_ONE_PER_WAVE)


def test_workgroup_kernel():
    """mpcqp_lds.hip (MPCQP_OPT_FORCE_LDS), (4, 2, 10, 3), 3 problems."""
    from qpmpc_amd import _capi

    discipline("workgroup kernel", ltv(810, 3, 4, 2, 10, 3, 0.3), flags=_capi.OPT_FORCE_LDS)


def test_mid_size_fused_kernel():
    """mpcqp_bigsolve.hip's fused front end (workspace: 2 n^2 elements per problem): the smallest row of
    tests/test_gpu_parity.py::test_mid_size_kernel_random_ltv_families, (12, 2, 16, 4), with MPCQP_OPT_FORCE_CONDENSED."""
    from qpmpc_amd import _capi

    discipline("mid-size", ltv(820, 3, 12, 2, 16, 4, 0.5), flags=_capi.OPT_FORCE_CONDENSED)


@pytest.mark.parametrize("tight", [1.0, 0.05])
def test_narrow_stagewise_and_its_second_opinion(tight):
    """mpcqp_stage.hip, (3, 1, 24, 2): the default dispatch; what it leaves unsolved goes to the wide kernel in the region behind
    its own. The default launch of the stage-wise entry point is the same pair of kernels."""
    # (whether a random draw at tight = 0.05 leaves an item to the wide kernel cannot be told from the outputs; the launch that
    # is sure to use the region behind the narrow kernel's is test_second_opinion_region_on_the_pinned_narrow_failure)
    w = ltv(830, 5, 3, 1, 24, 2, tight)
    case, out = discipline(f"narrow {tight}", w)
    assert case.ws_bytes > 0
    sw = Forward(w, stagewise=True)
    same_plans(out, sw.run(F), "mpcqp_stagewise_solve_batch launches the same kernels")


def test_second_opinion_region_on_the_pinned_narrow_failure():
    """tests/golden/second_opinion_narrow.npz ((4, 2, 26, 5): the narrow kernel alone ends MPCQP_MAX_ITER on it,
    tests/test_gpu_stateful_verdicts.py::test_second_opinion_solves_the_pinned_narrow_failure) as item 2 of five: this launch is
    sure to hand an item to the wide kernel, which works in the region behind the narrow kernel's."""
    z = np.load(os.path.join(HERE, "golden", "second_opinion_narrow.npz"))
    w = ltv(831, 5, 4, 2, 26, 5, 1.0)
    assert int(z["N"]) == 26 and (float(z["wt"]), float(z["wx"]), float(z["wu"])) == (w["wt"], w["wx"], w["wu"])
    for k in ("A", "B", "C", "D", "e", "x0", "goal", "targets"):
        w[k][2] = z[k][0]
    case, out = discipline("pinned second opinion", w)
    assert (out["status"] == 0).all(), out["status"]
    sw = Forward(w, stagewise=True)
    same_plans(out, sw.run(F), "mpcqp_stagewise_solve_batch launches the same kernels")


def test_narrow_stagewise_keep_then_reuse_factor():
    """MPCQP_OPT_KEEP_FACTOR under both fills; then MPCQP_OPT_REUSE_FACTOR, which reads the workspace by contract: the guards
    behind the queried size stay intact and the plans are the plain launch's, bitwise."""
    from qpmpc_amd import _capi

    w = ltv(830, 5, 3, 1, 24, 2, 1.0)
    case, kept = discipline("narrow keep", w, flags=_capi.OPT_KEEP_FACTOR)
    plain = case.run(F)
    equal_outputs(plain, kept, "keeping the factor changes nothing")
    for byte in (Z, F):
        case.run(byte, _capi.OPT_KEEP_FACTOR)
        again = case.run(byte, _capi.OPT_REUSE_FACTOR, keep=("ws",))
        equal_outputs(plain, again, f"reused factor, fill {byte:#04x}")


def test_wide_stagewise_float64():
    """mpcqp_stagew.hip, (6, 2, 20, 3) in float64: the default dispatch, equal to MPCQP_OPT_STAGE_WIDE of the stage-wise entry."""
    from qpmpc_amd import _capi

    w = ltv(840, 5, 6, 2, 20, 3, 0.5)
    case, out = discipline("wide f64", w)
    sw = Forward(w, stagewise=True)
    same_plans(out, sw.run(F, _capi.OPT_STAGE_WIDE), "mpcqp_stagewise_solve_batch launches the same kernel")


def test_wide_stagewise_float32_kernel():
    """BASELINE config 5's shape (12, 4, 64, mk = 16) in float32: the float32 stage-wise kernel (n = 256 > 160: not promoted)."""
    from qpmpc_amd import workloads as W

    discipline("wide f32", W.synthetic_ltv_batch(5), tol=1e-3, dtype=F32)


@pytest.mark.parametrize("shape", [(3, 1, 16, 2), (6, 2, 20, 3)])
@pytest.mark.parametrize("pad", [0, 7])
def test_float32_stored_float64_computed(shape, pad):
    """Float32 launches of at most 160 variables are converted into the workspace and solved in float64: the conversion region,
    with packed operands and with a batch stride 7 elements past the block (the padding holds the fill: NaN under fill F)."""
    w = ltv(850 + shape[0], 5, *shape, tight=0.5)
    case, out = discipline(f"promoted {shape} pad {pad}", w, tol=1e-3, dtype=F32, pad=pad)
    if pad:
        packed = Forward(w, dtype=F32)
        equal_outputs(out, packed.run(F), "a padded batch stride changes nothing")


def test_general_stagewise():
    """mpcqp_stageg.hip, (20, 6, 10, 4), 3 problems: the default dispatch, equal to MPCQP_OPT_STAGE_GENERAL of the stage-wise entry
    with the query at -1."""
    from qpmpc_amd import _capi

    w = ltv(860, 3, 20, 6, 10, 4, 0.5)
    case, out = discipline("general", w)
    sw = Forward(w, stagewise=True, query=-1)
    same_plans(out, sw.run(F, _capi.OPT_STAGE_GENERAL), "mpcqp_stagewise_solve_batch launches the same kernel")


@pytest.mark.parametrize("dtype,tol", [(F64, 1e-7), (F32, 1e-3)])
@pytest.mark.parametrize("extra", ["struct", "gws", "dense_g"])
def test_dense_hbm_path(dtype, tol, extra):
    """mpcqp_big.hip + mpcqp_bigsolve.hip on BASELINE config 5's shape, 2 problems: MPCQP_OPT_FORCE_CONDENSED alone (G applied
    through the roll-out), with MPCQP_OPT_FORCE_GWS and with MPCQP_OPT_FORCE_DENSE_G."""
    from qpmpc_amd import _capi
    from qpmpc_amd import workloads as W

    flags = _capi.OPT_FORCE_CONDENSED | {"struct": 0, "gws": _capi.OPT_FORCE_GWS, "dense_g": _capi.OPT_FORCE_DENSE_G}[extra]
    discipline("dense", W.synthetic_ltv_batch(2), tol=tol, dtype=dtype, flags=flags)


def test_cold_launch_with_a_warm_state_then_a_warm_launch():
    """(3, 1, 16, 2) with a warm state: the cold launch (warm_start = 0) under both fills writes the record; a warm launch from
    either record gives the same plans and iteration counts, bitwise. A warm launch begins from the stored operator, not from
    the empty set, so its plan equals the cold one to rounding only (1e-9 relative, the bound of
    tests/test_gpu_warm_start.py::test_warm_start_from_own_solution_needs_no_iteration)."""
    from qpmpc_amd import _capi

    w = ltv(870, 5, 3, 1, 16, 2, 0.3, "c", False)
    case = Forward(w, warm=True)
    warm, colds = {}, {}
    for byte in (Z, F):
        cold = colds[byte] = case.run(byte)
        against_oracle("warm cold", w, cold, 1e-7)
        warm[byte] = case.run(byte, warm_start=_capi.WARM_OPERATOR, keep=("warm",))
        against_oracle("warm warm", w, warm[byte], 1e-7)
        same_plans(cold, warm[byte], "warm launch on the same problem")
    equal_outputs(colds[Z], colds[F], "cold launches with a warm state: fill Z against fill F")
    equal_outputs(warm[Z], warm[F], "warm launches from the records of fill Z and fill F")
    ok = warm[Z]["status"] == 0
    assert (warm[Z]["iters"][ok] <= cold["iters"][ok]).all()


@pytest.mark.parametrize("shape", [(3, 2, 24, 3), (9, 4, 16, 4)])
def test_stagewise_entry_point(shape):
    """mpcqp_stagewise_solve_batch: default slots; max_active = 4 (items that need more end MPCQP_SLOTS_FULL); MPCQP_OPT_STAGE_WIDE;
    MPCQP_OPT_STAGE_GENERAL with the query at -1 and at -k."""
    from qpmpc_amd import _capi

    w = ltv(880 + shape[0], 5, *shape, tight=0.3)
    discipline(f"stagewise {shape}", w, stagewise=True)
    discipline(f"stagewise {shape}", w, stagewise=True, flags=_capi.OPT_STAGE_WIDE)
    discipline(f"stagewise {shape}", w, stagewise=True, flags=_capi.OPT_STAGE_GENERAL, query=-1)
    discipline(f"stagewise {shape}", w, stagewise=True, flags=_capi.OPT_STAGE_GENERAL, max_active=48, query=-48)
    # four slots: three items are at rest at their goal and targets (hardly a row active), the other two need more slots
    calm = ltv(890 + shape[0], 5, *shape, tight=4.0)
    calm["goal"][:3], calm["targets"][:3] = 0.0, 0.0
    _, few = discipline(f"stagewise four slots {shape}", calm, stagewise=True, max_active=4, skip_status=(_capi.SLOTS_FULL,))
    assert (few["status"] == _capi.SLOTS_FULL).any(), few["status"]


# ---------------------------------------------------------------------------------------------- condensing, dense solves

@pytest.mark.parametrize("name", ["small", "large_f64", "large_f32"])
def test_condense_and_its_phases(name):
    """mpcqp_condense_batch on chip ((3, 1, 16, 2), 5 problems) and through the workspace (BASELINE config 5's shape, 2 problems,
    both dtypes), Phi / Psi NULL and non-NULL; for the large ones also mpcqp_condense_phase_batch 1 then 2."""
    from qpmpc_amd import workloads as W

    _capi, lib, stream = _api()
    small = name == "small"
    w = W.triple_integrator_batch(5, seed=5) if small else W.synthetic_ltv_batch(2)
    dtype = F32 if name.endswith("f32") else F64
    bp = W.to_batch_problem(w, dtype=dtype)
    B, n, m, N, nx = bp.batch_size, bp.nb_variables, bp.nb_constraints, bp.nb_timesteps, bp.state_dim
    dims, nbytes = bp.dims(), C.c_size_t(0)
    assert lib.mpcqp_workspace_bytes(C.byref(dims), B, 0, C.byref(nbytes)) == 0
    print(f"    condense {name}: workspace {nbytes.value} bytes")
    L = Launch()
    add_problem(L, bp)
    for key, count in (("P", n * n), ("q", n), ("G", m * n), ("h", m), ("Phi", (N + 1) * nx * nx), ("Psi", (N + 1) * nx * n)):
        L.add(key, "out", dtype, B * count)
    L.add("ws", "scratch", U8, nbytes.value)
    L.build()
    cp = arena_problem(L, bp)

    def condense(prop):
        return lambda: lib.mpcqp_condense_batch(
            C.byref(dims), C.byref(cp), B, L.ptr("P"), L.ptr("q"), L.ptr("G"), L.ptr("h"), L.ptr("Phi") if prop else None,
            L.ptr("Psi") if prop else None, L.ptr("ws"), nbytes.value, stream())

    z1, z2, f = L.run(Z, condense(True)), L.run(Z, condense(True)), L.run(F, condense(True))
    for key in ("P", "q", "G", "h", "Phi", "Psi"):
        assert same_bits(z1[key], z2[key]), (key, "run to run")
        assert same_bits(z1[key], f[key]), (key, "fill Z against fill F")
    nn = L.run(F, condense(False))
    assert holds(nn["Phi"], F) and holds(nn["Psi"], F)
    for key in ("P", "q", "G", "h"):
        assert same_bits(nn[key], f[key]), (key, "Phi and Psi NULL")
    # (float32: the bound of tests/test_gpu_parity.py::test_config5_condense_mfma_gram_full_size, same shape and same measure)
    tol = 1e-12 if dtype == F64 else 2e-5
    refs = condense_refs(f32_view(w) if dtype == F32 else w, B)
    for b, cq in enumerate(refs):
        for key, want in (("P", cq.P), ("q", cq.q), ("G", cq.G), ("h", cq.h), ("Phi", np.vstack([cq.Phi, cq.phi_last])),
                          ("Psi", np.vstack([cq.Psi, cq.psi_last]))):
            got = f[key].reshape(B, -1)[b].astype(np.float64).reshape(want.shape)
            assert _rel(got, want) <= tol, (b, key, _rel(got, want))
    if small:
        return

    def phase(k):
        return lambda: lib.mpcqp_condense_phase_batch(
            C.byref(dims), C.byref(cp), B, k, L.ptr("P"), L.ptr("q"), L.ptr("G"), L.ptr("h"), L.ptr("Psi"), L.ptr("ws"),
            nbytes.value, stream())

    outs = {}
    for byte in (Z, F):
        one = L.run(byte, phase(1))
        assert holds(one["P"], byte) and holds(one["q"], byte) and holds(one["Phi"], byte)
        two = L.run(byte, phase(2), keep=("ws", "Psi", "G", "h"))
        assert holds(two["Phi"], byte)
        outs[byte] = two
    for key in ("P", "q", "G", "h", "Psi"):
        assert same_bits(outs[Z][key], outs[F][key]), (key, "phases: fill Z against fill F")
        assert same_bits(outs[F][key], f[key]), (key, "the two phases are the whole call")


@pytest.mark.parametrize("n,m,dtype,tol", [(10, 24, F64, 1e-7), (40, 90, F64, 1e-7), (96, 203, F32, 2e-3), (100, 300, F32, 2e-3),
                                           (160, 512, F64, 1e-8), (256, 1024, F32, 2e-3)])
def test_dense_qp_solver(n, m, dtype, tol):
    """mpcqp_solve_batch, 3 problems: the small-problem kernel (the size of test_solve_qp_batch_random_dense_qps), the workgroup
    kernel and the workspace-resident solver (every row of test_large_solver_dense_qps_vs_oracle, tolerances as there: the MFMA
    factor with m no multiple of 4, the scalar packed factor in float32 and float64, the blocked MFMA factor with 16-byte loads
    of G')."""
    B = 3
    P, q, G, h = _dense_qps(np.random.default_rng(n + m), B, n, m)
    c = QPs(P, q, G, h, dtype=dtype, workspace=True)
    print(f"    dense QP n {n} m {m}: workspace {c.ws_bytes} bytes")
    z1, z2, f = c.run(Z, 0), c.run(Z, 0), c.run(F, 0)
    equal_outputs(z1, z2, "run to run under fill Z")
    equal_outputs(z1, f, "fill Z against fill F")
    nn = c.run(F, 0, lam=False, iters=False)
    assert holds(nn["lam"], F) and holds(nn["iters"], F)
    equal_outputs(f, nn, "lam and iters NULL", lam=False, iters=False)
    ref = f32_view(dict(P=P, q=q, G=G, h=h)) if dtype == F32 else dict(P=P, q=q, G=G, h=h)
    solved = 0
    for b in range(B):
        xo, _, so, _ = oracle.gi_solve(ref["P"][b], ref["q"][b], ref["G"][b], ref["h"][b])
        assert (f["status"][b] == 0) == (so == 0)
        if so == 0:
            assert np.abs(f["U"][b].astype(np.float64) - xo).max() <= tol * max(1.0, np.abs(xo).max())
            solved += 1
    assert solved >= 2


def test_update_vectors_and_rollout():
    """mpcqp_update_vectors_batch with q or h NULL, and mpcqp_rollout_batch: the humanoid fixture's dimensions and (20, 6, 10, 4),
    3 problems, against oracle/condense_np.py (1e-12 relative)."""
    from qpmpc_amd import workloads as W

    _capi, lib, stream = _api()
    for w in (W.humanoid_batch(3, seed=3), ltv(900, 3, 20, 6, 10, 4, 0.5)):
        bp = W.to_batch_problem(w)
        B, n, m, N, nx = bp.batch_size, bp.nb_variables, bp.nb_constraints, bp.nb_timesteps, bp.state_dim
        dims = bp.dims()
        refs = condense_refs(w, B)
        rng = np.random.default_rng(5)
        Uin = rng.standard_normal((B, n))
        L = Launch()
        add_problem(L, bp)
        L.add("Phi", "in", F64, data=np.stack([np.vstack([c.Phi, c.phi_last]) for c in refs]))
        L.add("Psi", "in", F64, data=np.stack([np.vstack([c.Psi, c.psi_last]) for c in refs]))
        L.add("Uin", "in", F64, data=Uin)
        L.add("q", "out", F64, B * n)
        L.add("h", "out", F64, B * m)
        L.add("X", "out", F64, B * (N + 1) * nx)
        L.build()
        cp = arena_problem(L, bp)

        def update(q, h):
            return lambda: lib.mpcqp_update_vectors_batch(
                C.byref(dims), C.byref(cp), L.ptr("Phi"), (N + 1) * nx * nx, L.ptr("Psi"), (N + 1) * nx * n, B,
                L.ptr("q") if q else None, L.ptr("h") if h else None, stream())

        def rollout():
            return lib.mpcqp_rollout_batch(C.byref(dims), C.byref(cp.A), C.byref(cp.B), C.byref(cp.x0), L.ptr("Uin"), B, L.ptr("X"),
                                           stream())

        for byte in (Z, F):
            both = L.run(byte, update(True, True))
            assert holds(both["X"], byte)
            only_q, only_h = L.run(byte, update(True, False)), L.run(byte, update(False, True))
            assert holds(only_q["h"], byte) and holds(only_h["q"], byte)
            assert same_bits(only_q["q"], both["q"]) and same_bits(only_h["h"], both["h"])
            X = L.run(byte, rollout)
            assert holds(X["q"], byte) and holds(X["h"], byte)
            for b, cq in enumerate(refs):
                assert _rel(both["q"].reshape(B, n)[b], cq.q) <= 1e-12 and _rel(both["h"].reshape(B, m)[b], cq.h) <= 1e-12
                x, want = np.asarray(w["x0"][b], dtype=float), [np.asarray(w["x0"][b], dtype=float)]
                A, Bm = np.asarray(w["A"]), np.asarray(w["B"])
                for k in range(N):
                    Ak = A[b, k] if A.ndim == 4 else A
                    Bk = Bm[b, k] if Bm.ndim == 4 else Bm
                    x = Ak @ x + Bk @ Uin[b].reshape(N, -1)[k]
                    want.append(x)
                assert _rel(X["X"].reshape(B, -1)[b], np.concatenate(want)) <= 1e-12
            if byte == Z:
                first = (both, X)
        assert same_bits(first[0]["q"], both["q"]) and same_bits(first[0]["h"], both["h"]) and same_bits(first[1]["X"], X["X"])


# ---------------------------------------------------------------------------------------------- shared-model path
@pytest.mark.parametrize("family", ["triple", "wip12"])
def test_shared_model_factor_and_solves(family):
    """mpcqp_factor_model into a buffer of exactly mpcqp_model_bytes, then mpcqp_solve_model_batch (and _bounds_batch with bounds
    per problem) two and four per wavefront, 5 and 61 problems, against the oracle."""
    from qpmpc_amd import _capi
    from qpmpc_amd import workloads as W

    for batch in (5, 61):
        if family == "triple":
            w = W.triple_integrator_batch(batch, seed=batch, heterogeneous=False)
        else:
            w = W.wip_batch(batch, N=12, sampling_period=0.1, seed=5)
            w["x0"][: batch // 2, 1] += 0.4
            ts = np.stack([w["pendulum"].target_states(x, 0.5) for x in w["x0"]])
            w["goal"], w["targets"] = ts[:, -4:], ts[:, :-4]
        # the model's bounds are the workload's; every problem's own bounds are the same ones, stated per problem and per step
        N, mk = int(w["N"]), np.asarray(w["e"]).shape[-1]
        shared = dict(w, e_model=w["e"], e=np.broadcast_to(np.asarray(w["e"], dtype=float), (batch, N, mk)).copy())
        case = ModelCase(shared, factor_in_arena=True)
        print(f"    model {family} batch {batch}: model {case.model_bytes} bytes")
        for flags in (_capi.OPT_TWO_PER_WAVE, _capi.OPT_FOUR_PER_WAVE):
            for bounds in (False, True):
                what = f"model {family} {batch} flags {flags} bounds {bounds}"
                z1, z2, f = (case.run(byte, flags, bounds) for byte in (Z, Z, F))
                equal_outputs(z1, z2, what + ": run to run")
                equal_outputs(z1, f, what + ": fill Z against fill F")
                nn = case.run(F, flags, bounds, lam=False, iters=False)
                assert holds(nn["lam"], F) and holds(nn["iters"], F)
                equal_outputs(f, nn, what + ": lam and iters NULL", lam=False, iters=False)
                against_oracle(f"model {family} {batch}", w, f, 1e-7)


# ---------------------------------------------------------------------------------------------- derivative exports
VJP_CASES = [("condensed", (3, 2, 8, 2), 5, ()), ("model", (3, 2, 8, 2), 5, ()), ("stagewise", (3, 2, 8, 2), 5, ()),
             ("condensed", (4, 2, 64, 2), 2, ()), ("model", (4, 2, 64, 2), 2, ()), ("stagewise", (3, 2, 70, 2), 3, (1,))]


@pytest.mark.parametrize("kind,shape,batch,unsolved", VJP_CASES)
def test_plan_vjp_exports(kind, shape, batch, unsolved):
    """mpcqp_plan_vjp_batch / _vjp_model_batch / _vjp_stagewise_batch with every gradient asked for, then with the nullable ones
    NULL; one item of the long stage-wise case is handed over as unsolved (zeros and its status)."""
    nx, nu, N, mk = shape
    w = ltv(910 + N, batch, nx, nu, N, mk, 0.5)
    B = batch
    U, lam, status = forward_on_cpu(w, unsolved)
    p = PlanVjp(kind, shape, w, U, lam, status)
    L, gU, gX = p.L, p.gU, p.gX
    print(f"    vjp {kind} {shape} batch {B}: workspace {p.ws_bytes} bytes, max_active {p.ka}")
    z1, z2, f = L.run(Z, p.call()), L.run(Z, p.call()), L.run(F, p.call())
    for key in z1:
        if key != "ws":
            assert same_bits(z1[key], z2[key]), (key, "run to run under fill Z")
            assert same_bits(z1[key], f[key]), (key, "fill Z against fill F")
    _, vst = p.check(f, w, "packed")
    # the nullable pointers NULL (gX, every gradient but g_x0): their buffers keep the fill, g_x0 is that of gX = 0
    for byte in (Z, F):
        part = L.run(byte, p.call(full=False))
        for k in p.outs[1:]:
            assert holds(part["g_" + k], byte), (k, "was passed as NULL")
        assert np.array_equal(part["vjp_status"], vst)
        if byte == Z:
            first = part
    assert same_bits(first["g_x0"], part["g_x0"])
    for b in np.flatnonzero(vst == 0):
        w1 = AN.single(w, b)
        close(part["g_x0"].reshape(B, -1)[b], AN.vjp(w1, lam[b], gU[b], None)["x0"], (kind, b, "x0 without gX"))


JVP_CASES = [(False, False, (3, 2, 8, 2), 5, 1), (False, False, (3, 2, 8, 2), 5, 86),
             (True, False, (3, 2, 8, 2), 5, 1), (True, False, (3, 2, 8, 2), 5, 86),
             (False, True, (3, 2, 8, 2), 5, 1), (False, True, (3, 2, 70, 2), 3, 86), (False, True, (20, 6, 10, 4), 3, 13),
             (True, True, (3, 2, 8, 2), 5, 1), (True, True, (3, 2, 70, 2), 3, 86), (True, True, (20, 6, 10, 4), 3, 13)]


@pytest.mark.parametrize("model,stagewise,shape,batch,T", JVP_CASES)
def test_plan_jvp_exports(model, stagewise, shape, batch, T):
    """mpcqp_plan_jvp_batch / _jvp_stagewise_batch / _jvp_model_batch / _jvp_model_stagewise_batch: one tangent, and a ragged count
    one past 256 / max(nx, nu) (85 side by side for nx = 3, 12 for nx = 20: two passes over the slots, the second with one
    tangent); max_active as autodiff._max_active counts it; dX and jvp_status NULL next to the full call."""
    nx, nu, N, mk = shape
    w = ltv(930 + N, batch, nx, nu, N, mk, 0.5)
    B = batch
    unsolved = (1,) if N == 70 else ()
    U, lam, status = forward_on_cpu(w, unsolved)
    p = PlanJvp(model, stagewise, shape, w, U, lam, status, _tangents(w, B, T, np.random.default_rng(4), model))
    L = p.L
    print(f"    jvp model {model} stagewise {stagewise} {shape} batch {B} T {T}: workspace {p.ws_bytes} bytes, max_active {p.ka}")
    z1, z2, f = L.run(Z, p.call()), L.run(Z, p.call()), L.run(F, p.call())
    for key in ("dU", "dX", "jvp_status"):
        assert same_bits(z1[key], z2[key]), (key, "run to run under fill Z")
        assert same_bits(z1[key], f[key]), (key, "fill Z against fill F")
    which = range(T) if T <= 3 else (0, T // 2, T - 2, T - 1)  # (the last one is the second pass over the slots)
    p.check(f, w, "packed", which)
    part = L.run(F, p.call(full=False))
    assert holds(part["dX"], F) and holds(part["jvp_status"], F)
    assert same_bits(part["dU"], f["dU"]), "dX and jvp_status NULL"


# ---------------------------------------------------------------------------------------------- bookkeeping, closed loops
@pytest.mark.parametrize("batch", [1, 5, 1025])
def test_order_by_count(batch):
    """mpcqp_order_by_count with a workspace of exactly mpcqp_order_workspace_bytes: a permutation, longest first."""
    _, lib, stream = _api()
    counts = np.random.default_rng(batch).integers(0, 40, batch).astype(np.int32)
    nbytes = int(lib.mpcqp_order_workspace_bytes(batch))
    print(f"    order by count, batch {batch}: workspace {nbytes} bytes")
    L = Launch()
    L.add("counts", "in", I32, data=torch.as_tensor(counts))
    L.add("order", "out", I32, batch)
    L.add("ws", "scratch", U8, nbytes)
    L.build()

    def call():
        return lib.mpcqp_order_by_count(L.ptr("counts"), batch, L.ptr("order"), L.ptr("ws"), nbytes, stream())

    for byte in (Z, Z, F):
        order = L.run(byte, call)["order"]
        assert np.array_equal(np.sort(order), np.arange(batch)), "not a permutation"
        sorted_counts = counts[order]
        assert (np.diff(sorted_counts) <= 0).all(), "not sorted, longest first"


@pytest.mark.parametrize("mode", ["plain", "pipeline_factor", "reuse_factor"])
def test_wip_fused_periods(mode):
    """mpcqp_wip_period_batch / mpcqp_wip_periods_batch on W.wip_batch(5, N=50): the launch writes the plant's next state over
    `states` and the next problem over x0 / goal / targets, in place by contract. The first period (with MPCQP_OPT_KEEP_FACTOR in
    the factor-pipelining and factor-reusing sequences, as qpmpc_amd.closed_loop does) runs under both fills; it is the plain
    solve of the first problem followed by the reference's integrator. Then two more periods, which read what the first left
    in the workspace by contract: one launch each, against both in one launch -- bitwise equal, guards intact."""
    from qpmpc_amd import workloads as W
    from qpmpc_amd.closed_loop import NB_SUBSTEPS

    _capi, lib, stream = _api()
    B, N, T, vel = 5, 50, 0.024, 0.5
    w = W.wip_batch(B, N=N, seed=21)
    w["x0"][0], w["x0"][1] = [0.0, 0.3, 0.0, 1.0], [0.0, -0.25, 0.0, -0.8]  # (these two hold the input box active)
    pend = w["pendulum"]
    assert pend.nb_timesteps == N and pend.sampling_period == T
    ts = np.stack([pend.target_states(x, vel) for x in w["x0"]])
    w["goal"], w["targets"] = ts[:, -4:].copy(), ts[:, :-4].copy()
    bp = W.to_batch_problem(w)
    n, m, dims, nbytes = bp.nb_variables, bp.nb_constraints, bp.dims(), C.c_size_t(0)
    assert lib.mpcqp_workspace_bytes(C.byref(dims), B, 1, C.byref(nbytes)) == 0
    print(f"    wip periods {mode}: workspace {nbytes.value} bytes")
    L = Launch()
    add_problem(L, bp, inout=("x0", "goal", "targets"))
    L.add("states", "inout", F64, data=w["x0"])
    L.add("loop_stats", "inout", torch.int64, data=torch.zeros((B, 2), dtype=torch.int64))
    L.add("U", "out", F64, B * n)
    L.add("lam", "out", F64, B * m)
    L.add("status", "out", I32, B)
    L.add("iters", "out", I32, B)
    L.add("ws", "scratch", U8, nbytes.value)
    L.build()
    cp = arena_problem(L, bp)
    everything = tuple(s["name"] for s in L.specs)
    results = ("U", "lam", "status", "iters", "states", "loop_stats", "op_x0", "op_goal", "op_targets")

    def period(flags, slot, nperiods):
        o = _capi.SolveOpts()
        o.flags, o.factor_slot = int(flags), int(slot)
        head = (C.byref(dims), C.byref(cp), B, C.byref(o), L.ptr("U"), L.ptr("lam"), L.ptr("status"), L.ptr("iters"), L.ptr("ws"),
                nbytes.value, L.ptr("states"), L.ptr("loop_stats"), T, vel, float(pend.length), float(pend.GRAVITY), NB_SUBSTEPS)
        if nperiods is None:
            return lambda: lib.mpcqp_wip_period_batch(*head, stream())
        return lambda: lib.mpcqp_wip_periods_batch(*head, nperiods, stream())

    first_flags = 0 if mode == "plain" else _capi.OPT_KEEP_FACTOR

    def later(t):  # (flags, factor_slot) of period t >= 1
        if mode == "pipeline_factor":
            return _capi.OPT_PIPELINE_FACTOR, (t - 1) % 2
        return (_capi.OPT_REUSE_FACTOR if mode == "reuse_factor" else 0), 0

    z1, z2, f = (L.run(byte, period(first_flags, 0, None)) for byte in (Z, Z, F))
    for key in results:
        assert same_bits(z1[key], z2[key]), (key, "first period: run to run under fill Z")
        assert same_bits(z1[key], f[key]), (key, "first period: fill Z against fill F")
    several = L.run(F, period(first_flags, 0, 1))
    for key in results:
        assert same_bits(several[key], f[key]), (key, "mpcqp_wip_periods_batch of one period")
    against_oracle("wip first period", w, dict(U=f["U"].reshape(B, n), status=f["status"]), 1e-7)
    assert same_bits(f["op_x0"], f["states"]) and list(f["loop_stats"].reshape(B, 2)[:, 0]) == [0] * B
    assert np.array_equal(f["loop_stats"].reshape(B, 2)[:, 1], f["iters"]) and f["iters"][:2].min() > 0
    for b in range(B):
        x = np.asarray(w["x0"][b], dtype=float)
        for _ in range(NB_SUBSTEPS):
            x = np.asarray(pend.integrate(x, float(f["U"].reshape(B, n)[b, 0]), T / NB_SUBSTEPS), dtype=float)
        close(f["states"].reshape(B, 4)[b], x, ("wip plant", b))
    # periods 1 and 2, one launch each (everything stays as the launch before left it) ...
    for t in (1, 2):
        one = L.run(F, period(*later(t), None), keep=everything)
    # ... and both in one launch after the same first period
    L.run(F, period(first_flags, 0, None))
    two = L.run(F, period(*later(1), 2), keep=everything)
    for key in results:
        assert same_bits(one[key], two[key]), (key, "two periods in one launch against one launch each")
    assert not np.isnan(two["states"]).any() and (two["status"] == 0).all()


def test_wip_advance_with_a_padded_input_stride():
    """mpcqp_wip_advance_batch / _stats_batch on 5 loops: `states` is in/out by contract, U is read with u_stride > n and its
    padding holds the fill (NaN under fill F), status NULL and non-NULL; the plant step against the reference's integrator."""
    from qpmpc_amd import workloads as W
    from qpmpc_amd.systems import WheeledInvertedPendulum

    _capi, lib, stream = _api()
    B, N = 5, 50
    rng = np.random.default_rng(12)
    w = W.wip_batch(B, N=N)
    pend = WheeledInvertedPendulum(nb_timesteps=N, sampling_period=0.024)
    u_stride = N + 3
    Uin = 0.5 * rng.standard_normal((B, N))
    status = np.array([0, 0, 1, 0, 0], dtype=np.int32)
    L = Launch()
    L.add("states", "inout", F64, data=w["x0"])
    L.add("U", "in", F64, data=Uin, stride=u_stride)
    L.add("status", "in", I32, data=torch.as_tensor(status))
    L.add("iters", "in", I32, data=torch.as_tensor(np.arange(B, dtype=np.int32)))
    L.add("stats", "inout", torch.int64, data=torch.as_tensor(np.array([3, 4], dtype=np.int64)))
    L.add("x0", "out", F64, B * 4)
    L.add("goal", "out", F64, B * 4)
    L.add("targets", "out", F64, B * N * 4)
    L.build()
    phys = (N, 0.024, 0.5, float(pend.length), float(pend.GRAVITY), 4)

    def plain(st):
        return lambda: lib.mpcqp_wip_advance_batch(_capi.F64, L.ptr("states"), L.ptr("U"), u_stride, L.ptr("status") if st else None,
                                                   *phys, L.ptr("x0"), L.ptr("goal"), L.ptr("targets"), B, stream())

    def stats():
        return lib.mpcqp_wip_advance_stats_batch(_capi.F64, L.ptr("states"), L.ptr("U"), u_stride, L.ptr("status"), L.ptr("iters"),
                                                 L.ptr("stats"), *phys, L.ptr("x0"), L.ptr("goal"), L.ptr("targets"), B, stream())

    z, f, fs, nost = L.run(Z, plain(True)), L.run(F, plain(True)), L.run(F, stats), L.run(F, plain(False))
    for key in ("states", "x0", "goal", "targets"):
        assert same_bits(z[key], f[key]) and same_bits(f[key], fs[key]), key
    assert list(z["stats"]) == [3, 4] and list(fs["stats"]) == [4, 4 + int(np.arange(B).sum())]
    assert same_bits(f["states"].reshape(B, 4)[status == 0], nost["states"].reshape(B, 4)[status == 0])
    assert same_bits(f["x0"], f["states"]) and not np.isnan(f["targets"]).any() and not np.isnan(f["goal"]).any()
    moved = np.abs(f["states"].reshape(B, 4) - w["x0"]).max(axis=1)
    assert (moved > 0).all()
    # the reference's integrator on the same inputs (a zero input where the plan was not found)
    for b in range(B):
        x = np.asarray(w["x0"][b], dtype=float)
        u = 0.0 if status[b] else float(Uin[b, 0])
        for _ in range(4):
            x = np.asarray(pend.integrate(x, u, 0.024 / 4), dtype=float)
        close(f["states"].reshape(B, 4)[b], x, ("wip plant", b))


def _lipm_reference(states, U0, status, index, stride_index, support, strides, foot, N, T, nsub, nb_dsp, nb_ssp, free):
    """One period of the walkers in NumPy (qpmpc_amd.closed_loop.LIPMWalkingLoop's torch cross-check, itself the reference's
    integrate / PhaseStepper / update_goal_and_constraints): U0 None only writes the problem of the current phase."""
    states, index, stride_index, support = states.copy(), index.copy(), stride_index.copy(), support.copy()
    B = len(index)
    rows = np.arange(B)
    if U0 is not None:
        jerk = np.where(status == 0, U0, 0.0) if status is not None else U0
        dt = T / nsub
        p, v, a = states.T.copy()
        for _ in range(nsub):
            p, v, a = p + dt * (v + dt * (a / 2 + dt * jerk / 6)), v + dt * (a + dt * (jerk / 2)), a + dt * jerk
        states = np.stack([p, v, a], axis=1)
        nxt = support + strides[rows, stride_index]
        index = np.where(index + 1 >= nb_dsp + nb_ssp, 0, index + 1)
        support = np.where(index == 0, nxt, support)
        stride_index = np.where(index == 0, (stride_index + 1) % 2, stride_index)
    nxt = support + strides[rows, stride_index]
    last = nxt + strides[rows, (stride_index + 1) % 2]
    init_dsp = np.maximum(nb_dsp - index, 0)
    init_ssp = np.maximum(nb_ssp - np.maximum(index - nb_dsp, 0), 0)
    counts, left = [init_dsp, init_ssp], N - init_dsp - init_ssp
    for width in (nb_dsp, nb_ssp, nb_dsp, nb_ssp):
        counts.append(np.minimum(left, width))
        left = np.maximum(left - width, 0)
    counts = np.stack(counts, axis=1)
    ends = np.cumsum(counts, axis=1)
    seg = np.minimum((np.arange(N)[None, :, None] >= ends[:, None, :]).sum(axis=2), 5)
    half, fr = 0.5 * foot, np.full(B, free)
    upper = np.stack([fr, support + half, fr, nxt + half, fr, last + half], axis=1)
    lower = np.stack([fr, -(support - half), fr, -(nxt - half), fr, -(last - half)], axis=1)
    e = np.stack([np.take_along_axis(upper, seg, 1), np.take_along_axis(lower, seg, 1)], axis=2)
    goal = np.zeros((B, 3))
    goal[:, 0] = np.where(counts[:, 4] > 0, last, nxt)
    return dict(states=states, index=index, stride_index=stride_index, support=support, x0=states, goal=goal, e=e)


def test_lipm_advance():
    """mpcqp_lipm_advance_batch / _stats_batch on 5 walkers in different phases (two of them at the end of a step: the support
    foot changes): `states`, `index`, `stride_index` and `support` are in/out by contract and reloaded for each run, U is read with
    u_stride > n and its padding holds the fill, U NULL (only the current phase's problem is written) and non-NULL, status NULL
    and non-NULL, the stats variant; against the period restated in NumPy."""
    from qpmpc_amd.closed_loop import MAX_ZMP_DIST

    _capi, lib, stream = _api()
    B, N, T, nsub, nb_dsp, nb_ssp = 5, 16, 0.1, 15, 1, 7
    rng = np.random.default_rng(14)
    index = np.array([5, 0, 7, 3, 7], dtype=np.int64)
    stride_index = np.array([0, 1, 0, 1, 1], dtype=np.int64)
    support = np.array([0.09, -0.09, 0.09, 0.27, -0.2])
    strides = np.array([-0.18, 0.18]) * (1.0 + 0.2 * rng.random((B, 2)))
    foot = 0.065 * (1.0 + 0.3 * rng.random(B))
    omega = np.sqrt(9.81 / 0.84)
    states = np.stack([0.02 * rng.standard_normal(B), 0.5 * omega * support, -omega**2 * support], axis=1)
    u_stride = N + 3
    Uin = 2.0 * rng.standard_normal((B, N))
    status = np.array([0, 0, 1, 0, 0], dtype=np.int32)
    initial = dict(states=states, index=index, stride_index=stride_index, support=support)
    L = Launch()
    L.add("states", "inout", F64, data=states)
    L.add("index", "inout", torch.int64, data=torch.as_tensor(index))
    L.add("stride_index", "inout", torch.int64, data=torch.as_tensor(stride_index))
    L.add("support", "inout", F64, data=torch.as_tensor(support))
    L.add("strides", "in", F64, data=strides)
    L.add("foot", "in", F64, data=torch.as_tensor(foot))
    L.add("U", "in", F64, data=Uin, stride=u_stride)
    L.add("status", "in", I32, data=torch.as_tensor(status))
    L.add("iters", "in", I32, data=torch.as_tensor(np.arange(B, dtype=np.int32)))
    L.add("stats", "inout", torch.int64, data=torch.as_tensor(np.array([3, 4], dtype=np.int64)))
    L.add("x0", "out", F64, B * 3)
    L.add("goal", "out", F64, B * 3)
    L.add("e", "out", F64, B * N * 2)
    L.build()
    phys = (N, T, nsub, nb_dsp, nb_ssp, MAX_ZMP_DIST)
    tail = (L.ptr("index"), L.ptr("stride_index"), L.ptr("support"), L.ptr("strides"), L.ptr("foot"), L.ptr("x0"), L.ptr("goal"),
            L.ptr("e"), B)

    def plain(u, st):
        return lambda: lib.mpcqp_lipm_advance_batch(_capi.F64, L.ptr("states"), L.ptr("U") if u else None, u_stride,
                                                    L.ptr("status") if st else None, *phys, *tail, stream())

    def stats():
        return lib.mpcqp_lipm_advance_stats_batch(_capi.F64, L.ptr("states"), L.ptr("U"), u_stride, L.ptr("status"), L.ptr("iters"),
                                                  L.ptr("stats"), *phys, *tail, stream())

    keys = ("states", "index", "stride_index", "support", "x0", "goal", "e")
    shapes = dict(states=(B, 3), x0=(B, 3), goal=(B, 3), e=(B, N, 2))

    def check(out, ref, what, items=slice(None)):
        for key in keys:
            got = out[key].reshape(shapes.get(key, (B,)))[items]
            if got.dtype == np.int64:
                assert np.array_equal(got, ref[key][items]), (what, key, got, ref[key][items])
            else:
                close(got, ref[key][items], (what, key))

    args = (strides, foot, N, T, nsub, nb_dsp, nb_ssp, MAX_ZMP_DIST)
    z1, z2, f, fs = L.run(Z, plain(True, True)), L.run(Z, plain(True, True)), L.run(F, plain(True, True)), L.run(F, stats)
    for key in keys:
        assert same_bits(z1[key], z2[key]), (key, "run to run under fill Z")
        assert same_bits(z1[key], f[key]), (key, "fill Z against fill F")
        assert same_bits(f[key], fs[key]), (key, "the stats variant")
    assert list(f["stats"]) == [3, 4] and list(fs["stats"]) == [4, 4 + int(np.arange(B).sum())]
    ref = _lipm_reference(states, Uin[:, 0], status, index, stride_index, support, *args)
    assert (ref["index"] == 0).sum() == 2 and (ref["support"] != support).sum() == 2  # (two walkers change their support foot)
    check(f, ref, "one period")
    assert same_bits(f["x0"], f["states"])
    # status NULL: every plan counts as found (the walker whose status is 1 now moves by its own first jerk)
    outs = {byte: L.run(byte, plain(True, False)) for byte in (Z, F)}
    for key in keys:
        assert same_bits(outs[Z][key], outs[F][key]), (key, "status NULL: fill Z against fill F")
    check(outs[F], _lipm_reference(states, Uin[:, 0], None, index, stride_index, support, *args), "status NULL")
    ok = status == 0
    assert same_bits(outs[F]["states"].reshape(B, 3)[ok], f["states"].reshape(B, 3)[ok])
    # U NULL: nothing moves, the problem of the current phase is written
    outs = {byte: L.run(byte, plain(False, True)) for byte in (Z, F)}
    for key in keys:
        assert same_bits(outs[Z][key], outs[F][key]), (key, "U NULL: fill Z against fill F")
    for key, was in initial.items():
        assert same_bits(outs[F][key].reshape(was.shape), was), (key, "U NULL: the walker's state was written")
    check(outs[F], _lipm_reference(states, None, None, index, stride_index, support, *args), "U NULL")
