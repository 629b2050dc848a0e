"""GPU tests (-m gpu): every derivative export on degenerate active sets -- the cases of tests/degenerate_diff_cases.py, whose
inputs and references tests/test_degenerate_diff_cpu.py ties to the C oracle, to central differences and to long double.

Per (case, variant, export), nine problems per launch, seeded cotangents gU, gX and two seeded tangents per problem (those of e
move the two bounds of a pair together; the `_model` tangent exports add tangents of B and of the three weights):

  1  with the forward route's own multipliers (solve_mpc_batch, formulation="stagewise" for the stage-wise exports,
     SharedModel.solve with per-problem bounds for the shared-model ones): where the rows {lam > 0} are linearly independent
     (degenerate_diff_cases.independent: the rank test of CPU condition (e)) the status is 0 and every output matches the
     restatement at those same multipliers within 1e-8 max(1, |ref|), the tolerance the export's own tests hold it to; on
     `duplicate` and `band` the unique parts (x0, goal, targets, the pair-consistent part of e -- and of g_C, g_D -- g_A, g_B,
     g_w; dU and dX) also match the restatement at the oracle's canonical(lam), the derivative of the solution map of CPU
     condition (b); on `free`, items whose returned multipliers are all exactly zero give the unconstrained derivative. Where
     the rows are dependent the item is MPCQP_NOT_PD with zeros.
  2  on `duplicate`, with split(lam) injected (both members of every binding pair positive, a valid KKT multiplier vector with
     linearly dependent active rows), interleaved item by item with the same problems at canonical(lam) inside one launch of
     eighteen: an item with a binding pair is either MPCQP_NOT_PD with every output exactly zero, or status 0 with the unique
     parts within the same tolerance of the canonical reference, everything finite and no entry above 1e6 times the canonical
     reference's largest: status 0 with anything else fails, and each such item is named. The contract (include/mpcqp.h,
     DESIGN.md section 9) is the first outcome, and the launch is held to it: no item with a binding pair may come back with
     status 0 (the kernels of the parent commit returned status 0 on up to 5 of 9, right by cancellation). The neighbours at
     canonical(lam), and the split items without a binding pair, have status 0 and match.
  3  everywhere: no NaN or Inf in any output; an item the forward did not solve carries the forward's status and zeros -- the
     forward routes solve every item here, so the last neighbour of the interleaved launch is handed status MPCQP_INFEASIBLE
     and NaN multipliers, as tests/test_gpu_model_diff.py::test_mixed_wavefronts_status_passthrough_and_singular_problems does.

With MPCQP_DEGENERATE_DIFF_REPORT=<path> a complete run writes the table of profiles/degenerate_diff.txt."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import adjoint_model_np as AM
import adjoint_np as AN
import adjoint_stagewise_np as AS
import degenerate_cases as DC
import degenerate_diff_cases as DD
import model_adjoint_np as MN
import operand_layouts as OL
import tangent_model_np as TM
import tangent_model_stagewise_np as TMS
import tangent_np as TN
import tangent_stagewise_np as TS
from qpmpc_amd import workloads as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = OL.BATCH
TOL = 1e-8
NOT_PD = 3
BLOWUP = 1e6
FORCED_STATUS = 2  # MPCQP_INFEASIBLE, handed to one item of the interleaved launch
KEYS = ("x0", "goal", "targets", "e")
MODEL_KEYS = ("A", "B", "C", "D", "w")
ROWS = ("e", "C", "D")  # outputs with one entry (or one block) per constraint row: compared through degenerate_diff_cases.unique
PLAN_EXPORTS = {"condensed": ("plan_vjp", "plan_vjp_model", "plan_jvp", "plan_jvp_model"),
                "stagewise": ("plan_vjp_stagewise", "plan_jvp_stagewise", "plan_jvp_model_stagewise")}
MODEL_EXPORTS = ("model_vjp", "model_jvp")

PARAMS = []
for _kind, _shape in DD.CASES:
    if _kind == "model":
        _exports = MODEL_EXPORTS
    else:
        _exports = (PLAN_EXPORTS["condensed"] if _shape in DD.CONDENSED else ()) + (PLAN_EXPORTS["stagewise"] if _shape in DD.STAGEWISE else ())
    for _name in DD.VARIANTS:
        for _export in _exports:
            PARAMS.append(pytest.param(_kind, _shape, _name, _export, id=f"{DD.label(_kind, _shape)}-{_name}-{_export}"))
LABELS = [p.id for p in PARAMS]
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("MPCQP_DEGENERATE_DIFF_REPORT")
    if path and all(k in SEEN for k in LABELS):  # (a partial run, or -k, writes nothing)
        with open(path, "w") as fh:
            fh.write("tests/test_gpu_degenerate_diff.py, 9 problems per launch. Per case, variant (touch, free, duplicate, band:\n"
                     "tests/degenerate_cases.py) and export. Forward's own multipliers: the statuses the export returned, 0 / 3\n"
                     "(MPCQP_NOT_PD) counted; worst error against the restatement at those multipliers and, on duplicate and band,\n"
                     "of the unique parts against the restatement at the oracle's canonical(lam), both relative to\n"
                     "max(1, |ref|) (bound 1e-8); `both`: items where the forward returned both members of a pair positive;\n"
                     "`dep`: items whose rows {lam > 0} are linearly dependent; `weak`: touch / free items whose returned\n"
                     "multipliers include positive values below 1e-9. split(lam) injected (duplicate only): items with a binding\n"
                     "pair that came back 0 / MPCQP_NOT_PD, and the worst error of the status-0 items (those without a binding pair\n"
                     "included) and of the neighbours at canonical(lam). A case that missed an assertion is marked FAILED.\n\n")
            fh.write(f"{'case-variant-export':66s} {'own 0/3':>7s} {'own err':>8s} {'canon':>8s} {'both':>4s} {'dep':>3s} {'weak':>4s} "
                     f"{'split 0/3':>9s} {'split err':>9s} {'neighb':>8s}\n")
            for k in LABELS:
                s = SEEN[k]
                fh.write(f"{k:66s} {s['own']:>7s} {s['err']:8.1e} {s['canon']:>8s} {s['both']:4d} {s['dep']:3d} {s['weak']:>4s} "
                         f"{s['split']:>9s} {s['split_err']:>9s} {s['neigh']:>8s}{'' if s.get('passed') else '  FAILED'}\n")


# ---------------------------------------------------------------------------------------------- launches
def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _fake(U, lam, status):
    return SimpleNamespace(U=_t(U), multipliers=_t(lam), status=_t(status, torch.int32))


def _twice(w):
    """every problem of a materialised workload twice, the copies adjacent"""
    return {k: (np.repeat(v, 2, axis=0) if isinstance(v, np.ndarray) else v) for k, v in w.items()}


_FWD = {}


def _forward(kind, shape, name, stagewise):
    """(bp or SharedModel, U, lam, status) of the forward route on a variant, solved once"""
    key = (kind, shape, name, stagewise)
    if key not in _FWD:
        v = DD.variant(kind, shape, name)
        if kind == "model":
            from qpmpc_amd import SharedModel

            bp = W.to_batch_problem(DC.shared(v["w"]))
            prob = SharedModel(bp)
            plan = prob.solve(bp.initial_state, bp.goal_state, bp.target_states, return_multipliers=True, ineq_vector=_t(v["w"]["e"]))
        else:
            from qpmpc_amd import solve_mpc_batch

            prob = W.to_batch_problem(v["w"])
            plan = solve_mpc_batch(prob, return_multipliers=True, **(dict(formulation="stagewise") if stagewise else {}))
        torch.cuda.synchronize()
        _FWD[key] = (prob, plan.U.reshape(B, -1).cpu().numpy(), plan.multipliers.reshape(B, -1).cpu().numpy(), plan.status.cpu().numpy())
    return _FWD[key]


def _np(t, Bn):
    return None if t is None else t.reshape(Bn, -1).cpu().numpy()


def _launch(export, prob, shape, plan, gU, gX, tan, mtan):
    """(status [Bn], {output: [Bn, ...]}) of one export on `plan` (U, multipliers, status): gradients x0 .. e (and A .. D, w of
    the model kinds) or tangent responses U, X [Bn, T, ...]"""
    from qpmpc_amd import autodiff, model_diff

    nx, nu, N, mk = shape
    Bn = gU.shape[0]
    if export in ("plan_vjp", "plan_vjp_model", "plan_vjp_stagewise"):
        backward = dict(plan_vjp="condensed", plan_vjp_model="model", plan_vjp_stagewise="stagewise")[export]
        g = autodiff._vjp(prob, plan, _t(gU), _t(gX), set(KEYS) if backward == "condensed" else set(autodiff.GRAD_KEYS), backward)
        torch.cuda.synchronize()
        out = {k: _np(t, Bn) for k, t in zip(autodiff.GRAD_KEYS, g)}
        if backward != "condensed":
            out["w"] = np.stack([out.pop(k)[:, 0] for k in ("wt", "wx", "wu")], axis=1)
        return plan.vjp_status.cpu().numpy(), {k: a for k, a in out.items() if a is not None}
    if export == "model_vjp":
        g = model_diff.model_vjp(prob, plan, _t(gU), _t(gX), set(KEYS))
        torch.cuda.synchronize()
        return plan.vjp_status.cpu().numpy(), {k: _np(t, Bn) for k, t in zip(KEYS, g)}
    T = tan["x0"].shape[1]
    if export == "model_jvp":
        dU, dX = model_diff.model_jvp(prob, plan, _t(tan["x0"]), _t(tan["goal"]), _t(tan["targets"]), _t(tan["e"].reshape(Bn, T, N, mk)),
                                      states=True)
    else:
        model, weights = (None,) * 4, (None,) * 3
        if "model" in export:
            model = (None, _t(mtan["B"]), None, None)
            weights = tuple(_t(mtan["w"][:, :, i]) for i in range(3))
        dU, dX = autodiff._jvp(prob, plan, _t(tan["x0"]), _t(tan["goal"]), _t(tan["targets"]), _t(tan["e"].reshape(Bn, T, N, mk)), True,
                               "stagewise" if "stagewise" in export else "condensed", model, weights)
    torch.cuda.synchronize()
    return plan.jvp_status.cpu().numpy(), dict(U=dU.reshape(Bn, T, -1).cpu().numpy(), X=dX.reshape(Bn, T, -1).cpu().numpy())


# ---------------------------------------------------------------------------------------------- references
_MODEL = {}


def _reference(export, kind, shape, name, b, lam, U, gU, gX, tan, mtan):
    """{output: array} of the restatement of `export` on item b of a variant at multipliers lam and plan U (cotangents and
    tangents: the item's own)"""
    v = DD.variant(kind, shape, name)
    w1 = AN.single(v["w"], b)
    m = lam.size
    if export == "plan_vjp":
        return AN.vjp(w1, lam, gU, gX)
    if export == "plan_vjp_model":
        g, gm = AN.vjp(w1, lam, gU, gX), AM.model_vjp(w1, U, lam, gU, gX)
        return dict(g, **{k: gm[k] for k in MODEL_KEYS})
    if export == "plan_vjp_stagewise":
        g = AS.stagewise_vjp(w1, lam, gU, gX, U=U)
        assert g.pop("status") == 0
        return g
    if kind == "model":
        if (shape, name) not in _MODEL:
            _MODEL[(shape, name)] = MN.NumpyModel(DC.shared(v["w"]))
        model = _MODEL[(shape, name)]
        if export == "model_vjp":
            return model.vjp(lam, gU, gX)
        got = [model.jvp(lam, {k: a[t] for k, a in tan.items()}) for t in range(tan["x0"].shape[0])]
    else:
        got = []
        for t in range(tan["x0"].shape[0]):
            one = {k: a[t] for k, a in tan.items()}
            if "model" in export:
                one.update(B=mtan["B"][t], w=mtan["w"][t])
            got.append(dict(plan_jvp=lambda: TN.jvp(w1, lam, one), plan_jvp_stagewise=lambda: TS.stagewise_jvp(w1, lam, one),
                            plan_jvp_model=lambda: TM.jvp_model(w1, U, lam, one),
                            plan_jvp_model_stagewise=lambda: TMS.stagewise_jvp_model(w1, U, lam, one))[export]())
    return dict(U=np.stack([g["U"] for g in got]), X=np.stack([g["X"] for g in got]))


def _unique(key, a, pairs, m):
    """the part of output `key` that does not depend on how a binding pair shares its multiplier"""
    a = np.asarray(a, dtype=np.float64)
    if key in ROWS:
        return DD.unique(a.reshape(m, -1), pairs).ravel()
    return a.ravel()


class Err(float):
    """an error figure that remembers the output it was measured on"""
    key = "-"

    def __repr__(self):
        return f"{float(self):.2e} ({self.key})"


def _err(got, ref, pairs=None, m=0):
    """Err(worst over the outputs of |got - ref| / max(1, |ref|)), through _unique when `pairs` is given; .key names the output"""
    worst = Err(0.0)
    for key, r in ref.items():
        g = got[key]
        if pairs is not None:
            g, r = _unique(key, g, pairs, m), _unique(key, r, pairs, m)
        r = np.asarray(r, dtype=np.float64).ravel()
        if r.size:
            e = Err(float(np.abs(np.asarray(g).ravel() - r).max() / max(1.0, np.abs(r).max())))
            e.key = key
            worst = max(worst, e)
    return worst


def _item(out, b):
    return {k: a[b] for k, a in out.items()}


def _all_zero(out, b):
    return all((a[b] == 0).all() for a in out.values())


_CANON = {}


def _canonical_reference(export, kind, shape, name, b, gU, gX, tan, mtan):
    """the restatement at the oracle's canonical(lam) and plan, once per (export, case, variant, item)"""
    key = (export, kind, shape, name, b)
    if key not in _CANON:
        v = DD.variant(kind, shape, name)
        _CANON[key] = _reference(export, kind, shape, name, b, DD.canonical(v["lam"][b], v["pairs"]), v["U"][b], gU[b], gX[b],
                                 _item(tan, b), _item(mtan, b))
    return _CANON[key]


# ---------------------------------------------------------------------------------------------- the test
@pytest.mark.parametrize("kind,shape,name,export", PARAMS)
def test_export(kind, shape, name, export):
    nx, nu, N, mk = shape
    n, m = N * nu, N * mk
    label = f"{DD.label(kind, shape)}-{name}-{export}"
    v = DD.variant(kind, shape, name)
    pairs = v["pairs"]
    gU, gX = DD.cotangents(shape)
    tan, mtan = DD.tangents(shape, pairs), DD.model_tangents(shape)
    seen = SEEN[label] = dict(own="-", err=float("nan"), canon="-", both=0, dep=0, weak="-", split="-", split_err="-", neigh="-")

    # 1. the forward route's own multipliers
    prob, U, lam, fwd = _forward(kind, shape, name, "stagewise" in export)
    st, out = _launch(export, prob, shape, _fake(U, lam, fwd), gU, gX, tan, mtan)
    for key, a in out.items():
        assert np.isfinite(a).all(), (key, "NaN or Inf")  # 3
    seen["own"] = f"{int((st == 0).sum())}/{int((st == NOT_PD).sum())}"
    seen["both"] = sum(DD.both_positive(lam[b], pairs) > 0 for b in range(B))
    if name in ("touch", "free"):
        seen["weak"] = str(int(((lam > 0) & (lam < 1e-9)).any(axis=1).sum()))
    worst, worst_canon, failures = 0.0, 0.0, []
    for b in range(B):
        if fwd[b] != 0:  # 3
            assert st[b] == fwd[b] and _all_zero(out, b), (b, st[b], fwd[b])
            continue
        _, cq = DD.condensed_of(AN.single(v["w"], b))
        if not DD.independent(cq, lam[b]):
            seen["dep"] += 1
            if not (st[b] == NOT_PD and _all_zero(out, b)):
                failures.append((b, "dependent rows", int(st[b])))
            continue
        if st[b] != 0:
            failures.append((b, "status", int(st[b])))
            continue
        ref = _reference(export, kind, shape, name, b, lam[b], U[b], gU[b], gX[b], _item(tan, b), _item(mtan, b))
        e = _err(_item(out, b), ref)
        worst = max(worst, e)
        if e > TOL:
            failures.append((b, "own multipliers", e))
        if pairs:
            e = _err(_item(out, b), _canonical_reference(export, kind, shape, name, b, gU, gX, tan, mtan), pairs, m)
            worst_canon = max(worst_canon, e)
            if e > TOL:
                failures.append((b, "canonical(lam)", e))
        if name == "free" and (lam[b] == 0).all():
            e = _err(_item(out, b), _reference(export, kind, shape, name, b, np.zeros(m), U[b], gU[b], gX[b], _item(tan, b), _item(mtan, b)))
            if e > TOL:
                failures.append((b, "unconstrained", e))
    seen["err"] = worst
    if pairs:
        seen["canon"] = f"{worst_canon:.1e}"
    print(f"    {label}: own multipliers status {st.tolist()} error {worst:.1e} canonical {seen['canon']} both members positive on "
          f"{seen['both']} items, dependent rows on {seen['dep']}, weak {seen['weak']}")
    assert not failures, failures
    assert (fwd == 0).all(), fwd  # (the forward routes solve every item: tests/test_gpu_degenerate.py)

    # 2. split(lam) injected, interleaved with canonical(lam)
    if name == "duplicate":
        lam2 = np.empty((2 * B, m))
        lam2[0::2] = [DD.split(v["lam"][b], pairs) for b in range(B)]
        lam2[1::2] = [DD.canonical(v["lam"][b], pairs) for b in range(B)]
        twice = lambda a: np.repeat(a, 2, axis=0)  # noqa: E731
        if kind == "model":
            prob2 = prob
        else:
            prob2 = W.to_batch_problem(_twice(v["w"]))
        status2 = np.zeros(2 * B, dtype=np.int32)
        forced = 2 * B - 1  # the last neighbour comes with a forward status that says "not solved"; its multipliers are not read
        status2[forced], lam2[forced] = FORCED_STATUS, np.nan
        st2, out2 = _launch(export, prob2, shape, _fake(twice(v["U"]), lam2, status2), twice(gU), twice(gX),
                            {k: twice(a) for k, a in tan.items()}, {k: twice(a) for k, a in mtan.items()})
        for key, a in out2.items():
            assert np.isfinite(a).all(), (key, "NaN or Inf")
        passed, refused, worst_split, worst_neigh = 0, 0, 0.0, 0.0
        for b in range(B):
            ref = _canonical_reference(export, kind, shape, name, b, gU, gX, tan, mtan)
            bound = DD.binding(v["lam"][b], pairs)
            if 2 * b + 1 == forced:  # 3
                if not (st2[forced] == FORCED_STATUS and _all_zero(out2, forced)):
                    failures.append((b, "an unsolved item: the forward's status and zeros", int(st2[forced])))
            else:
                e = _err(_item(out2, 2 * b + 1), ref)
                worst_neigh = max(worst_neigh, e)
                if st2[2 * b + 1] != 0 or e > TOL:
                    failures.append((b, "neighbour at canonical(lam)", int(st2[2 * b + 1]), e))
            got = _item(out2, 2 * b)
            if st2[2 * b] == NOT_PD and bound:
                refused += 1
                if not _all_zero(out2, 2 * b):
                    failures.append((b, "MPCQP_NOT_PD without zeros"))
                continue
            if st2[2 * b] != 0:
                failures.append((b, "split status", int(st2[2 * b])))
                continue
            passed += bool(bound)
            e = _err(got, ref, pairs, m)
            worst_split = max(worst_split, e)
            big = max(float(np.abs(np.asarray(r)).max()) for r in ref.values() if np.asarray(r).size)
            blown = max(float(np.abs(a).max()) for a in got.values())
            if e > TOL or blown > BLOWUP * big:
                failures.append((b, "split(lam): status 0", e, blown, big))
        seen["split"], seen["split_err"], seen["neigh"] = f"{passed}/{refused}", f"{worst_split:.1e}", f"{worst_neigh:.1e}"
        print(f"    {label}: split(lam) items with a binding pair: {passed} status 0 (error {worst_split:.1e}), {refused} MPCQP_NOT_PD; "
              f"neighbours {worst_neigh:.1e}")
        assert not failures, failures
        assert passed + refused >= 6
        assert passed == 0, (passed, refused)  # the contract: every item with dependent active rows is refused
    seen["passed"] = True
