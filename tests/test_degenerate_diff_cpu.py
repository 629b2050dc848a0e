"""CPU tests: the inputs and references of tests/test_gpu_degenerate_diff.py are what tests/degenerate_diff_cases.py claims. For
every case (four plan shapes, three shared-model shapes), on the C oracle and in NumPy:

  (a) the oracle solves all nine items of every variant with status 0 in at most n + m iterations and its result passes
      kkt_certificate.certify; on `duplicate` and `band` at least 6 of 9 items have a binding pair (a positive multiplier on a
      member), and the oracle never puts a positive multiplier on both members; canonical(lam) and split(lam) pass the
      certificate too;
  (b) on `duplicate` and `band` the restatement adjoint_np.vjp at canonical(lam) equals central differences of the oracle
      (h = 1e-6) within the bound of tests/test_autodiff_cpu.py, 1e-6 max(1, |g|): x0, goal, targets entry by entry, e entry
      by entry off the pairs and along the direction that moves a pair's two bounds together (moving one member of a band alone
      makes the problem infeasible). The first two items with a binding pair of every case with n <= 40. Measured: 1.5e-8 at
      worst (plan (4, 2, 20, 2), duplicate), 3.4e-9 on the shared-model cases;
  (c) at lam, at canonical(lam) and with the multiplier moved to the other member the restatement's gradients agree in x0, goal,
      targets and the unique part of e. The margin is the rounding of two float64 KKT solves, each about cond(K) 2^-53 |g| off:
      measured 6.9e-15 max(1, |g|) at worst (plan (3, 2, 70, 2), duplicate; 0 wherever the oracle already had the multiplier on
      the first member), held to 1e-10, between that and the 1e-9 of condition (d);
  (d) every float64 restatement the GPU test compares against -- adjoint_np, adjoint_stagewise_np, model_adjoint_np for the
      gradients; tangent_np, tangent_stagewise_np, model_adjoint_np for the tangents -- is within 1e-9 max(1, |ref|), a tenth of
      the GPU tolerance, of the same KKT solve in np.longdouble (degenerate_diff_cases.vjp_ld / jvp_ld) at canonical(lam) on
      every item of every variant; the model gradients g_A .. g_D, g_w of adjoint_model_np and of adjoint_stagewise_np to
      degenerate_diff_cases.model_vjp_ld (the same long-double solve, long-double roll-outs). The restatement of the model
      tangents (tangent_model_np) has no long-double twin; it is held to the stage-wise restatement of the same quantity
      (tangent_model_stagewise_np), a different algorithm, at the same tenth;
  (e) at split(lam) the Gram matrix of the whitened active rows has numerical rank k - (number of binding pairs) (singular
      values relative to the largest, at 1e-12), and at canonical(lam) full rank."""
import numpy as np
import pytest

import adjoint_model_np as AM
import adjoint_np as AN
import adjoint_stagewise_np as AS
import degenerate_diff_cases as DD
import kkt_certificate as KC
import model_adjoint_np as MN
import operand_layouts as OL
import tangent_model_np as TM
import tangent_model_stagewise_np as TMS
import tangent_np as TN
import tangent_stagewise_np as TS

B = OL.BATCH
IDS = [DD.label(*c) for c in DD.CASES]
PAIRED = ("duplicate", "band")
KEYS = ("x0", "goal", "targets", "e")
TENTH = 1e-9  # a tenth of the GPU tolerance 1e-8 max(1, |ref|)


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


@pytest.mark.parametrize("name", DD.VARIANTS)
@pytest.mark.parametrize("kind,shape", DD.CASES, ids=IDS)
def test_oracle_solves_and_pairs_bind(kind, shape, name):
    """(a)"""
    nx, nu, N, mk = shape
    v = DD.variant(kind, shape, name)
    print(f"    {DD.label(kind, shape)}, {name}: status {v['status'].tolist()} iters {v['iters'].tolist()}")
    assert (v["status"] == 0).all(), v["status"]
    assert (v["iters"] <= N * nu + N * mk).all(), v["iters"]
    bad = [(b, str(c)) for b in range(B) for c in [KC.certify(v["w"], b, v["U"][b], v["lam"][b])] if not c.ok]
    assert not bad, bad
    if kind == "model":
        assert DD.DC.shared(v["w"])["C"].shape[0] == 1
    if name in PAIRED:
        bound = [len(DD.binding(v["lam"][b], v["pairs"])) for b in range(B)]
        assert sum(k > 0 for k in bound) >= 6, bound
        assert all(DD.both_positive(v["lam"][b], v["pairs"]) == 0 for b in range(B))
        for b in range(B):
            forms = [DD.canonical(v["lam"][b], v["pairs"])] + ([DD.split(v["lam"][b], v["pairs"])] if name == "duplicate" else [])
            for lam in forms:
                c = KC.certify(v["w"], b, v["U"][b], lam)
                assert c.ok, (b, str(c))
            if name == "duplicate":
                assert DD.both_positive(forms[1], v["pairs"]) == bound[b]


@pytest.mark.parametrize("name", PAIRED)
@pytest.mark.parametrize("kind,shape", [c for c in DD.CASES if c[1][1] * c[1][2] <= 40], ids=lambda x: str(x))
def test_restatement_at_canonical_is_the_derivative_of_the_solution_map(kind, shape, name):
    """(b)"""
    v = DD.variant(kind, shape, name)
    gU, gX = DD.cotangents(shape)
    items = [b for b in range(B) if DD.binding(v["lam"][b], v["pairs"])][:2]
    assert len(items) == 2
    worst = 0.0
    for b in items:
        w1 = AN.single(v["w"], b)
        ref = AN.vjp(w1, DD.canonical(v["lam"][b], v["pairs"]), gU[b], gX[b])
        ref["e"] = DD.unique(ref["e"], v["pairs"])
        second = {i1: (i0, f) for i0, i1, f in v["pairs"]}
        for key in KEYS:
            base = np.asarray(w1[key], dtype=float)
            g = np.zeros(base.size)
            for i in range(base.size):
                if key == "e" and i in second:
                    continue  # (moves with the pair's first member)
                vals = []
                for s in (1e-6, -1e-6):
                    pert = base.copy().ravel()
                    pert[i] += s
                    for i1, (i0, f) in second.items():
                        if key == "e" and i0 == i:
                            pert[i1] += f * s
                    vals.append(AN.loss(dict(w1, **{key: pert.reshape(base.shape)}), gU[b], gX[b]))
                g[i] = (vals[0] - vals[1]) / 2e-6
            err = _rel(g, ref[key])
            worst = max(worst, err)
            assert err <= 1e-6, (b, key, err)
    print(f"    {DD.label(kind, shape)}, {name}: items {items}, restatement at canonical(lam) against central differences {worst:.1e}")


@pytest.mark.parametrize("name", PAIRED)
@pytest.mark.parametrize("kind,shape", DD.CASES, ids=IDS)
def test_gradients_do_not_depend_on_the_member_that_carries_the_multiplier(kind, shape, name):
    """(c)"""
    v = DD.variant(kind, shape, name)
    gU, gX = DD.cotangents(shape)
    worst = 0.0
    for b in range(B):
        w1 = AN.single(v["w"], b)
        lam = v["lam"][b]
        got = []
        for form in (lam, DD.canonical(lam, v["pairs"]), DD.other(lam, v["pairs"])):
            g = AN.vjp(w1, form, gU[b], gX[b])
            g["e"] = DD.unique(g["e"], v["pairs"])
            got.append(g)
        for g in got[1:]:
            for key in KEYS:
                worst = max(worst, _rel(g[key], got[0][key]))
    print(f"    {DD.label(kind, shape)}, {name}: lam, canonical(lam) and the other member agree within {worst:.1e}")
    assert worst <= 1e-10, worst


def _tan(tan, b, t):
    return {k: a[b, t] for k, a in tan.items()}


@pytest.mark.parametrize("name", DD.VARIANTS)
@pytest.mark.parametrize("kind,shape", DD.CASES, ids=IDS)
def test_float64_restatements_against_long_double(kind, shape, name):
    """(d)"""
    v = DD.variant(kind, shape, name)
    gU, gX = DD.cotangents(shape)
    tan = DD.tangents(shape, v["pairs"])
    mtan = DD.model_tangents(shape)
    model = MN.NumpyModel(DD.DC.shared(v["w"])) if kind == "model" else None
    worst = {}

    def hold(what, got, ref):
        err = _rel(got, ref)
        worst[what] = max(worst.get(what, 0.0), err)
        assert err <= TENTH, (what, b, err)

    for b in range(B):
        w1 = AN.single(v["w"], b)
        lam = DD.canonical(v["lam"][b], v["pairs"])
        ld = DD.vjp_ld(w1, lam, gU[b], gX[b])
        refs = dict(adjoint_np=AN.vjp(w1, lam, gU[b], gX[b]))
        if kind == "model":
            refs["model_adjoint_np"] = model.vjp(lam, gU[b], gX[b])
        else:
            refs["adjoint_stagewise_np"] = sw = AS.stagewise_vjp(w1, lam, gU[b], gX[b], U=v["U"][b])
            assert sw["status"] == 0
            gm, gl = AM.model_vjp(w1, v["U"][b], lam, gU[b], gX[b]), DD.model_vjp_ld(w1, v["U"][b], lam, gU[b], gX[b])
            for key in ("A", "B", "C", "D", "w"):
                hold("adjoint_model_np " + key, gm[key], gl[key])
                hold("adjoint_stagewise_np " + key, sw[key], gl[key])
        for what, g in refs.items():
            for key in KEYS:
                hold(f"{what} {key}", g[key], ld[key])
        for t in range(tan["x0"].shape[1]):
            one = _tan(tan, b, t)
            jl = DD.jvp_ld(w1, lam, one)
            jrefs = dict(tangent_np=TN.jvp(w1, lam, one))
            if kind == "model":
                jrefs["model_adjoint_np jvp"] = model.jvp(lam, one)
            else:
                jrefs["tangent_stagewise_np"] = TS.stagewise_jvp(w1, lam, one)
                both = dict(one, B=mtan["B"][b, t], w=mtan["w"][b, t])
                jm, js = TM.jvp_model(w1, v["U"][b], lam, both), TMS.stagewise_jvp_model(w1, v["U"][b], lam, both)
                for key in ("U", "X"):
                    hold("tangent_model_np " + key, jm[key], js[key])
            for what, j in jrefs.items():
                for key in ("U", "X"):
                    hold(f"{what} {key}", j[key], jl[key])
    print(f"    {DD.label(kind, shape)}, {name}: " + ", ".join(f"{k} {e:.1e}" for k, e in worst.items()))


@pytest.mark.parametrize("kind,shape", DD.CASES, ids=IDS)
def test_split_multipliers_have_dependent_active_rows(kind, shape):
    """(e)"""
    v = DD.variant(kind, shape, "duplicate")
    for b in range(B):
        _, cq = DD.condensed_of(AN.single(v["w"], b))
        pairs = DD.binding(v["lam"][b], v["pairs"])
        act, S = DD.gram(cq, DD.split(v["lam"][b], v["pairs"]))
        assert DD.rank(S) == len(act) - len(pairs), (b, DD.rank(S), len(act), len(pairs))
        assert DD.independent(cq, DD.canonical(v["lam"][b], v["pairs"])) and not (pairs and DD.independent(cq, DD.split(v["lam"][b], v["pairs"])))
    vb = DD.variant(kind, shape, "band")
    for b in range(B):
        _, cq = DD.condensed_of(AN.single(vb["w"], b))
        assert DD.independent(cq, vb["lam"][b])
