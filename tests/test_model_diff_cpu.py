"""Shared-model derivatives without a GPU: the NumPy restatement of tests/model_adjoint_np.py against the condensed
restatements (tests/adjoint_np.py, tests/tangent_np.py), central differences of the C oracle and its own duality, on
four shared-operand families; and the C surface of mpcqp_model_vjp_batch / mpcqp_model_jvp_batch (header, binding,
library, host-side checks in their order)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adjoint_np as AN
import model_adjoint_np as MN
import tangent_np as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


FAMILIES = ("triple", "humanoid", "wip", "mixed")
_CACHE = {}


def _family(name):
    """(workload, NumPy model, oracle census), computed once per family."""
    if name not in _CACHE:
        w = MN.families()[name]
        _CACHE[name] = (w, MN.NumpyModel(w), MN.census(w))
    return _CACHE[name]


def _usable(name, count):
    _, _, cen = _family(name)
    return [b for b, c in enumerate(cen) if c[3]][:count]


def _close(got, ref, tol):
    return np.abs(np.asarray(got) - np.asarray(ref)).max() <= tol * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("name", FAMILIES)
def test_family_has_active_strictly_complementary_problems(name):
    _, _, cen = _family(name)
    assert sum(c[3] for c in cen) * 2 >= len(cen), (name, sum(c[3] for c in cen), len(cen))


@pytest.mark.parametrize("name", FAMILIES)
def test_vjp_restatement_matches_the_condensed_one(name):
    w, model, cen = _family(name)
    rng = np.random.default_rng(1)
    for b in _usable(name, 6):
        lam = cen[b][1]
        gU, gX = rng.standard_normal(model.n), rng.standard_normal((model.N + 1) * model.nx)
        w1 = AN.single(w, b)
        for gx in (None, gX):
            ref, got = AN.vjp(w1, lam, gU, gx), model.vjp(lam, gU, gx)
            for key in ("x0", "goal", "targets", "e"):
                assert _close(got[key], ref[key], 1e-9), (name, b, key)


@pytest.mark.parametrize("name", FAMILIES)
def test_vjp_restatement_matches_central_differences_of_the_oracle(name):
    w, model, cen = _family(name)
    rng = np.random.default_rng(2)
    for b in _usable(name, 2):
        gU, gX = rng.standard_normal(model.n), rng.standard_normal((model.N + 1) * model.nx)
        w1 = AN.single(w, b)
        fd, got = AN.fd_gradients(w1, gU, gX), model.vjp(cen[b][1], gU, gX)
        for key, ref in fd.items():
            assert _close(got[key], ref, 1e-6), (name, b, key, np.abs(got[key] - ref).max())


@pytest.mark.parametrize("name", FAMILIES)
def test_jvp_restatement_matches_the_condensed_one_and_the_vjp(name):
    w, model, cen = _family(name)
    rng = np.random.default_rng(3)
    for b in _usable(name, 6):
        lam = cen[b][1]
        w1 = AN.single(w, b)
        tan = TN.random_tangent(w1, rng)
        ref, got = TN.jvp(w1, lam, tan), model.jvp(lam, tan)
        assert _close(got["U"], ref["U"], 1e-9) and _close(got["X"], ref["X"], 1e-9), (name, b)
        gU, gX = rng.standard_normal(model.n), rng.standard_normal((model.N + 1) * model.nx)
        g = model.vjp(lam, gU, gX)
        fwd = np.concatenate([gU * got["U"], gX * got["X"]])
        rev = np.concatenate([g[k] * v for k, v in tan.items()])
        scale = max(1.0, np.abs(fwd).sum(), np.abs(rev).sum())
        assert abs(fwd.sum() - rev.sum()) <= 1e-10 * scale, (name, b)


def test_unflagged_terms_have_zero_maps():
    w = dict(MN.families()["triple"])  # terminal cost only: the targets do not enter q
    model = MN.NumpyModel(w)
    assert np.abs(model.Wt).max() == 0.0 and np.abs(model.Wg).max() > 0.0


# ---------------------------------------------------------------------------------------------- the C surface
NAMES = ("mpcqp_model_vjp_batch", "mpcqp_model_jvp_batch")


def _lib():
    from qpmpc_amd import _capi

    return _capi, _capi.load()


def test_exports_are_declared_bound_and_built():
    _capi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _capi.EXPORTS
        assert getattr(lib, name).argtypes is not None
    assert "#define MPCQP_ABI_VERSION 12" in header and lib.mpcqp_abi_version() == 12
    assert "mpcqp_model_vjp_batch / mpcqp_model_jvp_batch touch nothing outside" in header


def _dims(_capi, nx=3, nu=1, N=16, mk=2, dtype=None):
    return _capi.Dims(nx, nu, N, mk, _capi.F64 if dtype is None else dtype, _capi.P_TERMINAL | _capi.Q_TERMINAL,
                      1.0, 0.0, 1e-3)


def test_host_side_checks_in_their_order():
    """Every check returns its code with NULL or dummy device pointers: nothing is launched."""
    _capi, lib = _lib()
    EINVAL, EDTYPE, EUNSUPPORTED = -1, -3, -6
    p = 4096  # a dummy device address: never dereferenced by a call that fails its checks
    op = _capi.Operand(p, 0, 0)
    tan = _capi.Tangents(p, None, None, None, 0, 0, 0, 0)

    def vjp(d, model=p, batch=1, lam=p, status=p, gU=p, gX=None, A=None, B=None, g_x0=p):
        return lib.mpcqp_model_vjp_batch(C.byref(d), model, batch, lam, status, gU, gX, A, B, g_x0, None, None, None,
                                         None, None)

    def jvp(d, model=p, batch=1, ntan=1, lam=p, status=p, t=tan, A=None, B=None, dU=p, dX=None):
        return lib.mpcqp_model_jvp_batch(C.byref(d), model, batch, ntan, lam, status, None if t is None else C.byref(t),
                                         A, B, dU, dX, None, None)

    ok = _dims(_capi)
    for call in (vjp, jvp):
        # the dtype before everything else, then the envelope, then the arguments
        assert call(_dims(_capi, dtype=_capi.F32), model=None) == EDTYPE
        assert call(_dims(_capi, N=65), model=None) == EUNSUPPORTED
        assert call(ok, model=None) == EINVAL
        assert call(ok, status=None) == EINVAL
        assert call(ok, lam=None) == EINVAL
        assert call(ok, batch=-1) == EINVAL
        assert call(_dims(_capi, mk=0), lam=None, batch=0) == 0  # no rows: lam may be NULL; an empty batch launches nothing
    assert vjp(ok, gU=None) == EINVAL and vjp(ok, g_x0=None) == EINVAL
    assert vjp(ok, gX=p) == EINVAL and vjp(ok, gX=p, A=C.byref(op)) == EINVAL
    assert vjp(ok, gX=p, A=C.byref(op), B=C.byref(_capi.Operand(p, -1, 0))) == EINVAL
    assert vjp(ok, gX=p, A=C.byref(op), B=C.byref(op), batch=0) == 0
    assert jvp(ok, dU=None) == EINVAL and jvp(ok, t=None) == EINVAL
    assert jvp(ok, dX=p) == EINVAL and jvp(ok, dX=p, A=C.byref(op), B=C.byref(_capi.Operand(None, 0, 0))) == EINVAL
    assert jvp(ok, t=_capi.Tangents(p, None, None, None, -1, 0, 0, 0)) == EINVAL
    assert jvp(ok, ntan=0) == EINVAL and jvp(ok, ntan=257) == EINVAL
    assert jvp(ok, ntan=256, batch=0) == 0
    # a state so wide that the workgroup kernel's vectors do not fit a CU's LDS beside S (header: the envelope)
    wide = _dims(_capi, nx=12000, N=17)
    assert vjp(wide, model=None) == EUNSUPPORTED and jvp(wide, model=None) == EUNSUPPORTED
    assert vjp(_dims(_capi, nx=2000, N=17), model=None) == EINVAL


def test_python_envelope_is_refused_before_a_launch():
    from qpmpc_amd import BackendError, model_diff

    class _T:
        nb_variables = 65

    class _M:
        template = _T()

    with pytest.raises(BackendError, match="solve_mpc_batch_diff"):
        model_diff.check_envelope(_M())
