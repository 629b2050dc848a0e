"""What the fixtures tests/golden/quad_*_parent.npz share: each pins the outputs of the four-per-wavefront kernel
(csrc/mpcqp_quad.hip), U, lam, status and iters, to the bits recorded from an earlier build. The generators
tools/gen_golden_quad_{steady,drops,prologue,trip}.py keep what is theirs -- the operand sets, the seed search, the table of launches
and the conditions the fixture was chosen for --; tests/test_gpu_quad_parent_bits.py runs every launch of every table.

A fixture is a table {name: Launch}: the operand set a launch runs on and what is done to it (cut to its first problems, tiled past
the device's SIMDs, an iteration limit, a tolerance, padded batch strides, through a shared model). workload() is the NumPy workload
of a launch, run() what the kernel computes for it NOW, forced through MPCQP_OPT_FOUR_PER_WAVE; record() / stored() make a recording
(every launch twice with equal bits; of a tiled launch, whose tiles must repeat each other, the distinct results), pack() / unpack()
are the .npz layout, expand() / same_bits() the test's side. NumPy only at import: torch and qpmpc_amd are imported by what launches."""
from dataclasses import dataclass

import numpy as np

OPERANDS = ("A", "B", "C", "D", "e", "x0", "goal", "targets")
OUTPUTS = ("U", "lam", "status", "iters")
SCALARS = ("N", "wt", "wx", "wu")  # stored as float64, -1 for None
WAVE_PAST_SIMDS = "one wavefront more than the device has SIMDs"  # a tile count: the smallest launch of the slim LDS carve
_ATTR = dict(A="A", B="B", C="C", e="e", x0="initial_state", goal="goal_state")


@dataclass(frozen=True)
class Launch:
    on: str  # the operand set
    cut: int = None  # its first `cut` problems
    tile: object = None  # tiled to that many problems (a number, or WAVE_PAST_SIMDS) ...
    stored: int = None  # ... of which the fixture stores the first `stored` results: every tile must repeat them
    max_iter: int = None
    feas_tol: float = None
    pads: dict = None  # elements past the packed batch stride, per operand (padded())
    model: bool = False  # the set's x0 through a SharedModel of the humanoid problem


# ---------------------------------------------------------------------------------------------- workloads
def cut(w, count):
    out = dict(w)
    for k in OPERANDS:
        if isinstance(w.get(k), np.ndarray):
            out[k] = w[k][:count]
    return out


def tiled(w, count):
    out = dict(w)
    for k in OPERANDS:
        if isinstance(w.get(k), np.ndarray):
            v = w[k]
            out[k] = np.ascontiguousarray(np.concatenate([v] * (count // len(v) + 1))[:count])
    return out


def model_workload(x0):
    """the humanoid problem (qpmpc_amd.workloads.humanoid_matrices) from the initial states x0"""
    from qpmpc_amd import workloads as W

    w = W.humanoid_batch(len(x0))
    w["x0"] = x0
    return w


def count_of(spec, simds=None):
    """the problems of a tiled launch; simds: of the device, if not given (four per compute unit)"""
    if spec.tile != WAVE_PAST_SIMDS:
        return spec.tile
    if simds is None:
        import torch

        simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    return 4 * (simds + 1)


def workload(spec, sets, simds=None):
    """the NumPy workload of a launch: what goes to to_batch_problem (padded strides are made behind it)"""
    w = sets[spec.on]
    if spec.model:
        w = model_workload(w["x0"])
    if spec.cut:
        w = cut(w, spec.cut)
    if spec.tile:
        w = tiled(w, count_of(spec, simds))
    return w


# ---------------------------------------------------------------------------------------------- launches
def padded(bp, pads):
    """the batch problem with every per-problem operand named in `pads` moved behind a wider batch stride (NaN in the padding)"""
    import torch

    for key, pad in pads.items():
        t = getattr(bp, _ATTR[key])
        if t is None or t.shape[0] == 1 or not pad:
            continue
        block = t[0].numel()
        buf = torch.full((t.shape[0], block + pad), float("nan"), dtype=t.dtype, device=t.device)
        buf[:, :block] = t.reshape(t.shape[0], block)
        setattr(bp, _ATTR[key], buf[:, :block].view(t.shape))
        assert getattr(bp, _ATTR[key]).stride(0) == block + pad
    return bp


def _outputs(plan, probe=None):
    import torch

    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in (plan.U, plan.multipliers, plan.status, plan.iters))
    return out if probe is None else out + (probe.view(-1, 16).cpu().numpy(),)


def solve(w, *, max_iter=None, feas_tol=None, pads=None, probe=False):
    """(U, lam, status, iters) of the forced four-per-wavefront launch, as numpy arrays; with probe: and the [B, 16] probe record"""
    import torch
    from qpmpc_amd import _capi, solve_mpc_batch
    from qpmpc_amd import workloads as W

    bp = W.to_batch_problem(w)
    if pads:
        bp = padded(bp, pads)
    kw = {"probe": torch.zeros(bp.batch_size * 16, dtype=torch.int64, device=bp.device)} if probe else {}
    plan = solve_mpc_batch(bp, return_multipliers=True, max_iter=max_iter, feas_tol=feas_tol, flags=_capi.OPT_FOUR_PER_WAVE, **kw)
    return _outputs(plan, kw.get("probe"))


def solve_model(x0, *, max_iter=None, feas_tol=None):
    """the same through a shared model factored from the humanoid problem"""
    from qpmpc_amd import SharedModel, _capi
    from qpmpc_amd import workloads as W

    bp = W.to_batch_problem(model_workload(x0))
    plan = SharedModel(bp).solve(bp.initial_state, bp.goal_state, bp.target_states, return_multipliers=True, max_iter=max_iter,
                                 feas_tol=feas_tol, flags=_capi.OPT_FOUR_PER_WAVE)
    return _outputs(plan)


def run(spec, sets):
    """what the kernel computes NOW for a launch (a tiled one: all its problems)"""
    if spec.model:
        return solve_model(sets[spec.on]["x0"], max_iter=spec.max_iter, feas_tol=spec.feas_tol)
    return solve(workload(spec, sets), max_iter=spec.max_iter, feas_tol=spec.feas_tol, pads=spec.pads)


# ---------------------------------------------------------------------------------------------- recording and comparing
def expand(want, count):
    """the recorded results repeated to `count` problems: what every tile of a tiled launch must give"""
    return tuple(np.concatenate([v] * (count // len(v) + 1))[:count] for v in want)


def fold_tiles(results, distinct, count):
    """the first `distinct` results of a tiled launch of `count` problems, every tile of which must repeat them bit for bit"""
    first = tuple(v[:distinct] for v in results)
    for v, ref in zip(results, expand(first, count)):
        assert len(v) == count and ref.tobytes() == v.tobytes(), "slim tiles differ"
    return first


def record(run, names):
    """{name: run(name)}, every name run twice with equal bits (the kernel is deterministic)"""
    results = {name: run(name) for name in names}
    again = {name: run(name) for name in names}
    for name in names:
        for a, b in zip(results[name], again[name]):
            assert a.tobytes() == b.tobytes(), name
    return results


def stored(launches, results):
    """the results a fixture stores: of a tiled launch the distinct ones (fold_tiles)"""
    return {name: fold_tiles(res, launches[name].stored, count_of(launches[name])) if launches[name].tile else res
            for name, res in results.items()}


def report(results):
    for name, res in results.items():
        print(f"{name:13s} statuses {np.bincount(res[2], minlength=4)} iters mean {res[3].mean():.2f} max {res[3].max()}")


def pack(sets, results, out_prefix="out_", **extras):
    """the arrays of a fixture file: {set}__{operand} (scalars as float64, -1 for None), {launch}__{out_prefix}{output}, the extras"""
    out = dict(extras)
    for name, w in sets.items():
        for k in OPERANDS:
            if isinstance(w.get(k), np.ndarray):
                out[f"{name}__{k}"] = w[k]
        for k in SCALARS:
            if k in w:
                out[f"{name}__{k}"] = np.float64(-1.0 if w[k] is None else w[k])
    for name, res in results.items():
        for k, v in zip(OUTPUTS, res):
            out[f"{name}__{out_prefix}{k}"] = v
    return out


def unpack(z, operand_sets, result_sets, out_prefix="out_"):
    """(operand dictionaries by set, recorded outputs by launch) of a loaded fixture file"""
    sets, results = {}, {}
    for name in operand_sets:
        w = {k: (z[f"{name}__{k}"] if f"{name}__{k}" in z.files else None) for k in OPERANDS}
        for k in SCALARS:
            if f"{name}__{k}" in z.files:
                v = float(z[f"{name}__{k}"])
                w[k] = int(v) if k == "N" else (None if v < 0 else v)
        sets[name] = w
    for name in result_sets:
        results[name] = tuple(z[f"{name}__{out_prefix}{k}"] for k in OUTPUTS)
    return sets, results


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if a.tobytes() != b.tobytes():
        raw = np.dtype(f"u{a.dtype.itemsize}")
        bad = np.flatnonzero((a.view(raw) != b.view(raw)).reshape(len(a), -1).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} problems differ from the parent's bits, first {bad[:8].tolist()}")
