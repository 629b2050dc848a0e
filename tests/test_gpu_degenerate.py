"""GPU tests (-m gpu): every forward route on degenerate active sets -- the problems of tests/degenerate_cases.py, on which the
linear-dependence, ratio-test and drop branches of a dual active-set kernel decide the outcome and the answer is known all the
same (tests/test_degenerate_cases_cpu.py shows on the C oracle that the inputs are what they claim to be):

  touch      the bound of every row that is inactive at the optimum moved onto the optimum, rounded outward: exact ties, fully
             and over-determined vertices. Exact answer: the nominal problem's plan.
  free       every bound moved onto the unconstrained minimiser u0: nothing is active, every row ties. Exact answer: u0.
  duplicate  a row stated twice, and a row stated again at twice its scale, both binding. Reference: the oracle on the variant.
  band       a row and its exact negative with bounds e and -e: an equality written as two inequalities. Reference: the oracle.

Launched as tests/test_gpu_verdicts.py launches its cases (Forward of tests/guarded_launch.py, the route's flags and
dtype, fill 0xFF), nine problems per launch. Per launch: return code 0, status 0 for all nine, iters written, no NaN; the plan
within the route's bound (1e-7 float64, 1e-3 float32, scaled as against_oracle scales it) of the exact answer or the oracle's;
on `free`, float64 routes whose rounding bound n 2^-53 sum_j |G_ij u0_j| / (1 + |h_i|) is at most 1e-13 on every row (a tenth of
feas_tol) report iters == 0 -- a kernel that admits a row sitting on the minimiser compares against the wrong scale -- on every
item whose rows a float64 minimiser keeps within a twentieth of feas_tol (degenerate_cases.FREE_SLACK, the rule of condition (e)
of tests/test_degenerate_cases_cpu.py). That is narrower than "all nine": the rounding bound counts the evaluation of a slack,
not the minimiser's own error, about cond(P) 2^-53 |u|. On item 8 of "quad lean" / "pair lean" (cond(P) = 3.5e4, no stage cost)
that error is 4e-12, the kernels take one iteration and the C oracle two, all three returning u0 within 5e-13;
on float64 routes every item whose NOMINAL launch passes kkt_certificate.certify passes it on the variant too (the multipliers
are not unique here, so they are never compared with the oracle's), and on `band` the equality holds two-sided,
|G_0 u - h_0| / (1 + |h_0|) <= 1e-9.

The same assertions on the shared-model export (two and four per wavefront), the dense-QP export (every size of
verdict_cases.DENSE_SIZES) and the on-chip 17 .. 32-variable kernel (csrc/mpcqp_duo.hip) in its three modes.

With MPCQP_DEGENERATE_REPORT=<path> a complete run writes the table of profiles/degenerate_active_sets.txt."""
import os

import numpy as np
import pytest

import degenerate_cases as DC
import kkt_certificate as KC
import onchip32_cases as OC
import operand_layouts as OL
import verdict_cases as VC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import guarded_launch as GL  # noqa: E402  (the arena launchers; needs torch)
from guarded_launch import Forward, ModelCase, QPs  # noqa: E402
from guarded_launch import flags as _flags  # noqa: E402

F, F64, F32, I32, U8 = GL.F, GL.F64, GL.F32, GL.I32, GL.U8
LD = np.longdouble
ROUTES, VARIANTS = list(OL.ROUTES), list(DC.VARIANTS)
FREE_ROUNDING = 1e-13  # a tenth of the default feas_tol of include/mpcqp.h

SEEN = {}  # (label, variant) -> what the report prints
PASSED = set()
LABELS = []  # every (label, variant) the file launches, in order

# Failures found by this file on an MI355X and not fixed yet: (label, variant) -> route, variant, observed status and error, each an
# xfail(strict=True): a case that starts to pass must leave the table. It held `touch` at four dense-QP sizes -- MPCQP_INFEASIBLE on
# solvable problems after 379 .. 1645 iterations, every slot taken and |z|^2 up to 13 |M_p|^2 where it must vanish. Since
# csrc/mpcqp_bigsolve.hip rebuilds its operator T when it has visibly lost its accuracy, 160 x 512 float64 (1.2e-13, nine
# certificates) and 96 x 203 float32 (2.0e-4) are solved; the two float32 sizes below are not, for another reason.
_DENSE_F32 = ("dense QP {0} float32, touch: status {1} (1 MPCQP_MAX_ITER, 2 MPCQP_INFEASIBLE, on solvable problems; the oracle solves "
              "all nine in at most {2} iterations), largest iters {3}. With T rebuilt the loop no longer diverges, but at the "
              "over-determined vertex ({4} of n rows active, 45 .. 56 more through the optimum) the float32 slacks of the touched "
              "rows are noise of either sign above row_tol = 1e-5 (|G_i| + |h_i|): rows are admitted and dropped in turn (a NumPy "
              "restatement of the loop in float32 takes 1,100 .. 13,000 iterations on such items) until a dependent row meets only "
              "non-positive ratios or the acceptance test finds the active rows off their bounds. Needs a tie rule for rows within "
              "noise of the vertex in the float32 dense kind; the other items of each size are solved within the bound.")
XFAIL = {
    ("dense QP 100 x 300 f32", "touch"): _DENSE_F32.format("100 x 300", "210100002", 378, 4010, "96 .. 98"),
    ("dense QP 256 x 1024 f32", "touch"): _DENSE_F32.format("256 x 1024", "110000100", 957, 1620, "251 .. 256"),
}


def _params(label_of, cases):
    """every case x every variant as pytest params, the ones of XFAIL marked xfail(strict=True)"""
    out = []
    for case in cases:
        for name in VARIANTS:
            why = XFAIL.get((label_of(*case), name))
            out.append(pytest.param(*case, name, marks=[pytest.mark.xfail(strict=True, reason=why)] if why else [],
                                    id=f"{label_of(*case)}-{name}"))
    return out


def _label(label):
    for name in VARIANTS:
        LABELS.append((label, name))
    return label


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("MPCQP_DEGENERATE_REPORT")
    if path and all(k in SEEN for k in LABELS):  # (a partial run, or -k, writes nothing)
        with open(path, "w") as fh:
            fh.write("tests/test_gpu_degenerate.py, 9 problems per launch, fill 0xFF. Per launch and variant (touch, free, duplicate,\n"
                     "band: tests/degenerate_cases.py): the statuses; the largest iteration count of the nominal launch and of the\n"
                     "variant, and the largest ratio variant / nominal over the nine items (items with a nominal count of 0 left\n"
                     "out; 'free' has no nominal counterpart: its counts alone, '=0/k' where the test holds k of the nine items to zero); the error\n"
                     "against the exact answer (touch, free) or the oracle on the variant (duplicate, band), scaled by\n"
                     "max(1, |reference|_inf) per problem (bound: 1e-7 float64, 1e-3 float32, the dense QPs' own); certificates\n"
                     "held / eligible (items whose nominal launch passes tests/kkt_certificate.py; float64 only). A case that\n"
                     "missed an assertion is marked FAILED (xfail: a known failure, listed first).\n\n")
            for k, why in XFAIL.items():
                fh.write(f"known failure (xfail, strict): {why}\n")
            fh.write("\n")
            fh.write(f"{'launch':46s} {'variant':9s} {'status':9s} {'it nom':>6s} {'it var':>6s} {'ratio':>6s} {'error':>8s} {'certified':>9s}\n")
            for k in LABELS:
                s = SEEN[k]
                fh.write(f"{k[0]:46s} {k[1]:9s} {s['status']:9s} {s['it_nom']:6d} {s['it_var']:>6s} {s['ratio']:>6s} {s['err']:8.1e} "
                         f"{s['cert']:>9s}{'' if k in PASSED else '  FAILED (xfail)' if k in XFAIL else '  FAILED'}\n")


def _rel(U, ref):
    return float((np.abs(U.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))).max())


def _judge(label, name, out, base, v, ref, tol, f64, certify, equality, f64_slack):
    """the assertions of the module docstring on one launch `out` of variant `name`. base: (outputs, certified [B] bool) of the
    same launch on the nominal problems; v: the variant (degenerate_cases); ref: the plan it is held to; certify(b, U, lam) ->
    Certificate on the variant's operands; equality(U) -> |G_0 u - h_0| / (1 + |h_0|) [B] of the banded row, in long double;
    f64_slack(b) -> the smallest scaled slack of item b at a float64 minimiser (degenerate_cases.min_slack_f64)."""
    nom, cert = base
    st, it, U = out["status"], out["iters"].astype(np.int64), out["U"]
    itn = nom["iters"].astype(np.int64)
    finite = not np.isnan(U).any()
    err = _rel(U, ref) if finite else float("nan")
    held, lost = 0, []
    if f64 and cert.any() and finite and (st == 0).all():
        for b in np.flatnonzero(cert):
            c = certify(int(b), U[b], out["lam"][b])
            held += int(c.ok)
            if not c.ok:
                lost.append((int(b), str(c)))
    zero = np.zeros(len(st), dtype=bool)  # the items of `free` held to 0 iterations
    if name == "free" and f64 and float(v["bound"].max()) <= FREE_ROUNDING:
        zero = np.array([f64_slack(b) >= DC.FREE_SLACK for b in range(len(st))])
    ratio = float((it[itn > 0] / itn[itn > 0]).max()) if name != "free" and (itn > 0).any() else float("nan")
    SEEN[(label, name)] = dict(status="".join(str(int(s)) for s in st), it_nom=int(itn.max()), it_var=f"{int(it.max())}{'=0/' + str(int(zero.sum())) if zero.any() else ''}",
                               ratio="-" if np.isnan(ratio) else f"{ratio:.2f}", err=err,
                               cert=f"{held}/{int(cert.sum())}" if f64 else "-")
    print(f"    {label}, {name}: status {st.tolist()} iters {it.tolist()} (nominal {itn.tolist()}) error {err:.2e} certificates "
          f"{held} of {int(cert.sum())}" + (f", rounding bound {float(v['bound'].max()):.1e}, held to 0 iterations: items {np.flatnonzero(zero).tolist()}" if name == "free" else ""))
    assert (st == 0).all(), st
    assert (it >= 0).all(), it
    assert finite
    assert err <= tol, err
    assert (it[zero] == 0).all(), (it, zero, float(v["bound"].max()))
    assert not lost, lost
    if name == "band" and f64:
        eq = equality(U)
        print(f"    {label}, band: |G_0 u - h_0| / (1 + |h_0|) {float(eq.max()):.1e}")
        assert (eq <= KC.PRIMAL).all(), eq
    PASSED.add((label, name))


def _certified(U, lam, certify):
    return np.array([certify(b, U[b], lam[b]).ok for b in range(len(U))])


def _band_row(w):
    """equality(U) of a workload variant: the banded row is row 0 of step N // 2"""
    k = int(w["N"]) // 2

    def equality(U):
        e = w["e"][:, k, 0].astype(LD)
        return np.abs(DC.row_values(w, U.astype(np.float64))[:, k, 0] - e) / (1 + np.abs(e))

    return equality


def _workload_case(label, name, key, full, steps, f32, launch, tol):
    """one variant of nine MPC problems through launch(w) -> outputs; the nominal launch is made once per label"""
    if label not in _BASE:
        nom = launch(full)
        assert (nom["status"] == 0).all(), nom["status"]
        cert = np.zeros(OL.BATCH, dtype=bool)
        if not f32:  # (float32 multipliers do not reach the certificate's 1e-9)
            cert = _certified(nom["U"].astype(np.float64), nom["lam"].astype(np.float64), lambda b, U, lam: KC.certify(full, b, U, lam))
        _BASE[label] = (nom, cert)
    v = DC.case_variant(key, full, name, steps, f32)
    w = v["w"]
    ref = v["exact"] if v["exact"] is not None else DC.oracle_on(key, name, w)[0]
    out = launch(w)
    _judge(label, name, out, _BASE[label], v, ref, tol, not f32, lambda b, U, lam: KC.certify(w, b, U, lam), _band_row(w),
           lambda b: DC.min_slack_f64(w, b))


_BASE = {}


# ---------------------------------------------------------------------------------------------- every route of OL.ROUTES
for _r in ROUTES:
    _label(_r)


@pytest.mark.parametrize("route,name", _params(lambda route: route, [(r,) for r in ROUTES]))
def test_route(route, name):
    r = OL.ROUTES[route]
    key, (_, full) = OL.route_case(route, 0)

    def launch(w):
        case = Forward(w, dtype=F32 if r["f32"] else None, stagewise=r["stagewise"])
        assert case.B == OL.BATCH
        return case.run(F, _flags(r["flags"]))

    _workload_case(route, name, key, full, DC.TOUCH_STEPS[route], r["f32"], launch, 1e-3 if r["f32"] else 1e-7)


# ---------------------------------------------------------------------------------------------- the shared-model export
def _model_launch(flag):
    def launch(w):
        return ModelCase(DC.shared(w)).run(F, _flags([flag]))

    return launch


MODEL = [(shape, flag) for shape in OL.MODEL_SHAPES for flag in ("OPT_TWO_PER_WAVE", "OPT_FOUR_PER_WAVE")]
for _shape, _flag in MODEL:
    _label(f"model {_shape} {_flag}")


@pytest.mark.parametrize("shape,flag,name", _params(lambda shape, flag: f"model {shape} {flag}", MODEL))
def test_shared_model(shape, flag, name):
    """mpcqp_factor_model + mpcqp_solve_model_bounds_batch on variant 0 of OL.model_case: duplicate and band are rows of the shared
    model, e is per problem"""
    _workload_case(f"model {shape} {flag}", name, ("model", shape), OL.model_case(shape, 0)[1], None, False, _model_launch(flag), 1e-7)


# ---------------------------------------------------------------------------------------------- the dense-QP export
def _dense_launch(P, q, G, h, f32, flags, workspace):
    return QPs(P, q, G, h, dtype=F32 if f32 else F64, workspace=workspace).run(F, flags)


def _dense_case(label, name, n, m, f32, tol, flags, workspace):
    if label not in _BASE:
        P, q, G, h = DC.dense_nominal(n, m, f32)
        nom = _dense_launch(P, q, G, h, f32, flags, workspace)
        assert (nom["status"] == 0).all(), nom["status"]
        cert = np.zeros(OL.BATCH, dtype=bool)
        if not f32:
            cert = _certified(nom["U"], nom["lam"], lambda b, U, lam: KC.certify_qp(P[b], q[b], G[b], h[b], U, lam))
        _BASE[label] = (nom, cert)
    v = DC.dense_variant(n, m, f32, name)
    P, q, G, h = v["qp"]
    ref = v["exact"] if v["exact"] is not None else DC.dense_oracle(("dense", n, m, f32, name), P, q, G, h)[0]
    out = _dense_launch(P, q, G, h, f32, flags, workspace)

    def equality(U):
        r = np.einsum("bj,bj->b", G[:, 0].astype(LD), U.astype(LD)) - h[:, 0].astype(LD)
        return np.abs(r) / (1 + np.abs(h[:, 0]))

    _judge(label, name, out, _BASE[label], v, ref, tol, not f32, lambda b, U, lam: KC.certify_qp(P[b], q[b], G[b], h[b], U, lam), equality,
           lambda b: DC.min_slack_qp(P[b], q[b], G[b], h[b]))


def _dense_label(n, m, f32, tol=None):
    return f"dense QP {n} x {m} {'f32' if f32 else 'f64'}"


for _size in VC.DENSE_SIZES:
    _label(_dense_label(*_size))


@pytest.mark.parametrize("n,m,f32,tol,name", _params(_dense_label, VC.DENSE_SIZES))
def test_dense_qp(n, m, f32, tol, name):
    """mpcqp_solve_batch at every size of tests/test_gpu_memory_discipline.py::test_dense_qp_solver: touch on h, duplicate and band on
    rows 0 and 1 of G; the bound is the size's own (verdict_cases.DENSE_SIZES)"""
    _dense_case(_dense_label(n, m, f32), name, n, m, f32, tol, 0, True)


# ---------------------------------------------------------------------------------------------- the on-chip 17 .. 32-variable kernel
for _shape in DC.ONCHIP_SHAPES:
    _label(f"on chip, fused {_shape}")
for _shape in DC.ONCHIP_SHAPES:
    _label(f"on chip, model {_shape}")
for _n, _m in DC.ONCHIP_QP_SIZES:
    _label(f"on chip, QP {_n} x {_m}")


@pytest.mark.parametrize("shape,name", _params(lambda shape: f"on chip, fused {shape}", [(s,) for s in DC.ONCHIP_SHAPES]))
def test_onchip_fused(shape, name):
    """MPCQP_OPT_ON_CHIP_32 through mpcqp_build_solve_batch, without a workspace, on the nine general problems of
    tests/test_gpu_onchip32.py::test_verdicts"""
    assert tuple(OC.VERDICT_SHAPES) == tuple(DC.ONCHIP_SHAPES)

    def launch(w):
        return Forward(w, workspace=False).run(F, _flags(["OPT_ON_CHIP_32"]))

    _workload_case(f"on chip, fused {shape}", name, ("on chip", shape), DC.onchip_full(shape), None, False, launch, 1e-7)


@pytest.mark.parametrize("shape,name", _params(lambda shape: f"on chip, model {shape}", [(s,) for s in DC.ONCHIP_SHAPES]))
def test_onchip_model(shape, name):
    """its shared-model mode, at the verdict shapes of tests/onchip32_model_cases.py"""
    import onchip32_model_cases as MC

    assert tuple(MC.VERDICT_SHAPES) == tuple(DC.ONCHIP_SHAPES)
    _workload_case(f"on chip, model {shape}", name, ("model", shape), OL.model_case(shape, 0)[1], None, False,
                   _model_launch("OPT_ON_CHIP_32"), 1e-7)


@pytest.mark.parametrize("n,m,name", _params(lambda n, m: f"on chip, QP {n} x {m}", DC.ONCHIP_QP_SIZES))
def test_onchip_qp(n, m, name):
    """its QP-given mode, at onchip32_qp_cases.CROSS_ROUTE, without a workspace"""
    import onchip32_qp_cases as QC

    assert tuple(QC.CROSS_ROUTE) == tuple(DC.ONCHIP_QP_SIZES)
    _dense_case(f"on chip, QP {n} x {m}", name, n, m, False, QC.TOL, _flags(["OPT_ON_CHIP_32"]), False)
