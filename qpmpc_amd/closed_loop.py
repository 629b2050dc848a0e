"""Receding-horizon closed loops on the device (BASELINE config 3).

Batched counterpart of the loop in the reference's
examples/wheeled_inverted_pendulum.py:99-118: at every MPC step each loop
(1) rebuilds its reference ramp from its current state (:65-83, :101-108),
(2) builds and solves its MPC problem -- one fused launch for the whole batch,
replacing the per-step ``solve_mpc`` call (:109) -- and (3) applies the first
input to the nonlinear plant for NB_SUBSTEPS Taylor sub-steps (:110-111,
qpmpc/systems/wheeled_inverted_pendulum.py:127-160). States, references and
inputs stay in HBM; the host only enqueues work.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

import ctypes as C

from . import _capi
from .batch import BatchMPCProblem, PreparedSolve, SharedModel, WarmState, _dtype_code, _stream_ptr
from .exceptions import BackendError
from .systems import WheeledInvertedPendulum

NB_SUBSTEPS = 15  # examples/wheeled_inverted_pendulum.py:31


def wip_problem(pendulum: WheeledInvertedPendulum, x0, ltv: bool = True, dtype=None, device=None) -> BatchMPCProblem:
    """Batch of WIP problems (weights of the reference example, :90-94) for states x0 [B,4]."""
    A, B = pendulum.discretized_dynamics()
    N = pendulum.nb_timesteps
    if ltv:  # "LTV = pass A, B as N-lists" 
        A = np.ascontiguousarray(np.broadcast_to(A, (N, 4, 4)))
        B = np.ascontiguousarray(np.broadcast_to(B, (N, 4, 1)))
    D = np.array([[1.0], [-1.0]])
    e = np.array([pendulum.max_ground_accel, pendulum.max_ground_accel])
    x0 = np.asarray(x0, dtype=float)
    ts = np.stack([pendulum.target_states(x, 0.0) for x in x0])
    return BatchMPCProblem(A, B, None, D, e, N, 10.0, 1.0, 1e-3, x0, goal_state=ts[:, -4:],
                           target_states=ts[:, :-4], dtype=dtype, device=device)


class WIPClosedLoop:
    """``B`` independent wheeled-inverted-pendulum control loops advancing in lock step."""

    def __init__(self, x0, nb_timesteps: int = 50, sampling_period: float = 0.024, target_vel: float = 0.5,
                 ltv: bool = True, max_iter: Optional[int] = None, shared_model: bool = False, fused_period: bool = True,
                 reuse_factor: bool = False, pipeline_factor: bool = False, periods_per_launch: int = 1):
        """``fused_period``: run a whole period (solve + plant + next problem + bookkeeping) in ONE launch,
        ``mpcqp_wip_period_batch``, where the solver kernel supports it (else, and with ``shared_model``, two
        launches per period). ``reuse_factor``: the dynamics and weights never change along the loop, so the
        stage-wise kernel keeps its Riccati factor in the workspace after the first period and starts from it
        afterwards (``MPCQP_OPT_KEEP_FACTOR`` / ``MPCQP_OPT_REUSE_FACTOR``: build once, re-solve -- the reference's
        ``update_cost_vector`` / ``update_constraint_vector`` usage; ignored by kernels that rebuild anyway).
        ``pipeline_factor``: the factor is REBUILT every period, like the reference's ``solve_mpc`` does, but by a second
        wavefront that works on the next period's factor while the first one solves this period with the factor the
        previous launch left (``MPCQP_OPT_PIPELINE_FACTOR``; the operands of the next period are known here: they do
        not change). Same trajectories, bit for bit; falls back to the plain rebuilding period where the kernel does
        not offer it. ``periods_per_launch``: with the fused period, ``step(n)`` runs up to that many consecutive periods
        per launch (``mpcqp_wip_periods_batch``: the wavefront that solved period t carries on with period t + 1; the
        loops never interact, so nothing has to meet at a period's end) -- same trajectories bit for bit, without the
        dispatch gap between the periods. The first period of an episode is always a launch of its own.

        HIP graphs: with ``reuse_factor`` and ``pipeline_factor`` off and ``periods_per_launch=1`` the steady-state
        ``step(1)`` makes the same call(s) every period and can be captured once (after the first periods ran eagerly) and
        replayed: tests/test_gpu_streams.py does so with the fused one-launch period (24 timesteps) and with the two
        launches per period the loop falls back to where the fused one is not offered (12 timesteps).
        ``reuse_factor`` switches its flags after the first period and ``pipeline_factor`` alternates ``factor_slot`` with the host-side period count: their periods differ from one
        another in host-side state, so a captured period is not replayable by construction."""
        import torch

        self.pendulum = WheeledInvertedPendulum(nb_timesteps=nb_timesteps, sampling_period=sampling_period)
        self.problem = wip_problem(self.pendulum, x0, ltv=ltv)
        self.target_vel = float(target_vel)
        # shared_model=True: the dynamics, constraints and weights never change along the
        # loop, so P, its factor and M are computed ONCE (SharedModel) instead of at every
        # step; False reproduces the reference, which rebuilds everything per step
        # (solve_mpc.py:42).
        if shared_model:
            self.solver = SharedModel(self.problem).prepare(self.problem, max_iter=max_iter)
        else:
            self.solver = PreparedSolve(self.problem, max_iter=max_iter)
        self.states = self.problem.initial_state.clone()
        N, T = nb_timesteps, sampling_period
        dev, dt = self.states.device, self.states.dtype
        # ramp[k] = k*T*target_vel for k = 0..N (reference position offsets)
        self._ramp = torch.arange(N + 1, device=dev, dtype=dt) * (T * self.target_vel)
        self.mpc_steps = 0
        self._stats = torch.zeros((2,), dtype=torch.int64, device=dev)  # [failed, sum of iterations], mpcqp_accumulate_stats
        # per-loop [failed, iterations] counters of the fused period (no atomics in the solver kernel's epilogue);
        # the public counters ``failed`` / ``iters_total`` (properties below) add both
        self._loopstats = torch.zeros((self.problem.batch_size, 2), dtype=torch.int64, device=dev)
        self._fused = bool(fused_period) and not shared_model  # cleared by the first launch if the kernel cannot do it
        self._period_args = None
        self._ppl = max(1, int(periods_per_launch))
        self._reuse = bool(reuse_factor) and not shared_model
        self._pipe = bool(pipeline_factor) and not shared_model and not self._reuse
        if self._reuse or self._pipe:
            self.solver._opts.flags |= _capi.OPT_KEEP_FACTOR

    def _write_references(self) -> None:
        """target_states / goal_state / initial_state of every loop from its current state, in place (so the bound
        pointers stay valid): one launch of the plant kernel with zero sub-steps (``mpcqp_wip_advance_batch``, nsub = 0)."""
        p, pend = self.problem, self.pendulum
        rc = _capi.load().mpcqp_wip_advance_batch(
            _dtype_code(p.dtype), self.states.data_ptr(), self.solver.U.data_ptr(), p.nb_variables, None, pend.nb_timesteps,
            pend.sampling_period, self.target_vel, pend.length, pend.GRAVITY, 0, p.initial_state.data_ptr(),
            p.goal_state.data_ptr(), p.target_states.data_ptr(), p.batch_size, _stream_ptr())
        _capi.check(rc, "mpcqp_wip_advance_batch")

    def _write_references_torch(self) -> None:
        """The same with torch operations (kept as a cross-check of the kernel: tests/)."""
        p, N = self.problem, self.pendulum.nb_timesteps
        pos = self.states[:, 0:1] + self._ramp[None, :]  # [B, N+1]
        tgt = p.target_states.view(-1, N, 4)
        tgt.zero_()
        tgt[:, :, 0] = pos[:, :N]
        tgt[:, :, 2] = self.target_vel
        p.goal_state.zero_()
        p.goal_state[:, 0] = pos[:, N]
        p.goal_state[:, 2] = self.target_vel
        p.initial_state.copy_(self.states)

    def reset(self, x0) -> None:
        """Put every loop back to state ``x0`` [B, 4] (a new episode; counters restart)."""
        import torch

        self.states.copy_(torch.as_tensor(np.asarray(x0, dtype=float), dtype=self.states.dtype, device=self.states.device))
        self.mpc_steps = 0
        self._stats.zero_()
        self._loopstats.zero_()
        # (the kept factor stays valid across episodes: it depends on the dynamics and the weights only)

    @property
    def failed(self):
        """0-d int64 device tensor: periods of any loop whose plan was not found, whichever launch counted them
        (the two-launch period's global counter + the fused period's per-loop counters)."""
        return self._stats[0] + self._loopstats[:, 0].sum()

    @property
    def iters_total(self):
        """0-d int64 device tensor: active-set iterations of all solves so far."""
        return self._stats[1] + self._loopstats[:, 1].sum()

    def step(self, nb_mpc_steps: int = 1):
        """Advance every loop by ``nb_mpc_steps`` MPC periods: per period one solver launch
        and one fused plant + reference + bookkeeping launch (``mpcqp_wip_advance_stats_batch``). Asynchronous."""
        lib = _capi.load()
        p, pend = self.problem, self.pendulum
        if self.mpc_steps == 0:
            self._write_references()
        left = int(nb_mpc_steps)
        while left > 0:
            left -= 1
            if self._reuse and self.mpc_steps == 1:  # the first period of the episode left the factor in the workspace
                self.solver._opts.flags = (self.solver._opts.flags & ~_capi.OPT_KEEP_FACTOR) | _capi.OPT_REUSE_FACTOR
            if self._pipe:
                o = self.solver._opts
                if self.mpc_steps == 0:  # the first period factors for itself and keeps the factor in image 0
                    o.flags = (o.flags & ~_capi.OPT_PIPELINE_FACTOR) | _capi.OPT_KEEP_FACTOR
                    o.factor_slot = 0
                else:  # period t solves with image (t - 1) % 2 while the factor for period t + 1 goes into image t % 2
                    o.flags = (o.flags & ~_capi.OPT_KEEP_FACTOR) | _capi.OPT_PIPELINE_FACTOR
                    o.factor_slot = (self.mpc_steps - 1) % 2
            if self._fused:
                if self._period_args is None:  # converted once: the call is launch-rate-bound otherwise
                    import ctypes as C

                    self._period_args = tuple(self.solver._args) + (
                        C.c_void_p(self.states.data_ptr()), C.c_void_p(self._loopstats.data_ptr()),
                        C.c_double(pend.sampling_period), C.c_double(self.target_vel), C.c_double(pend.length),
                        C.c_double(pend.GRAVITY), C.c_int32(NB_SUBSTEPS))
                # periods of this launch: the episode's first period stands alone (it keeps its factor for the others)
                k = 1 if self.mpc_steps == 0 else min(self._ppl, left + 1)
                rc = lib.mpcqp_wip_periods_batch(*self._period_args, k, _stream_ptr())
                if rc == _capi.EUNSUPPORTED and self._pipe and self.mpc_steps > 0:
                    # (this horizon has no factor image to pipeline through: plain rebuilding periods)
                    self._pipe = False
                    self.solver._opts.flags &= ~(_capi.OPT_PIPELINE_FACTOR | _capi.OPT_KEEP_FACTOR)
                    rc = lib.mpcqp_wip_periods_batch(*self._period_args, k, _stream_ptr())
                if rc == _capi.EUNSUPPORTED and k > 1:
                    # (this horizon has no multi-period instantiation; the fused single-period launch may still exist)
                    self._ppl = k = 1
                    rc = lib.mpcqp_wip_periods_batch(*self._period_args, k, _stream_ptr())
                if rc == _capi.EUNSUPPORTED:
                    self._fused = False  # (another kernel serves this size: two launches per period)
                else:
                    _capi.check(rc, "mpcqp_wip_periods_batch")
                    self.mpc_steps += k
                    left -= k - 1
                    continue
            if self._pipe:
                rc = self.solver._entry(*self.solver._args, _stream_ptr())
                if rc == _capi.EUNSUPPORTED:  # (a kernel without factor images serves this size: plain rebuilds)
                    self._pipe = False
                    self.solver._opts.flags &= ~(_capi.OPT_PIPELINE_FACTOR | _capi.OPT_KEEP_FACTOR)
                    rc = self.solver._entry(*self.solver._args, _stream_ptr())
                _capi.check(rc, "mpcqp_build_solve_batch")
            else:
                self.solver.launch()
            rc = lib.mpcqp_wip_advance_stats_batch(
                _dtype_code(p.dtype), self.states.data_ptr(), self.solver.U.data_ptr(), p.nb_variables,
                self.solver.status.data_ptr(), self.solver.iters.data_ptr(), self._stats.data_ptr(), pend.nb_timesteps,
                pend.sampling_period, self.target_vel, pend.length, pend.GRAVITY, NB_SUBSTEPS, p.initial_state.data_ptr(),
                p.goal_state.data_ptr(), p.target_states.data_ptr(), p.batch_size, _stream_ptr())
            _capi.check(rc, "mpcqp_wip_advance_stats_batch")
            self.mpc_steps += 1
        return self.states

    def stats(self) -> Dict[str, float]:
        B = self.problem.batch_size
        solves = max(self.mpc_steps * B, 1)
        return {
            "loops": B,
            "mpc_steps": self.mpc_steps,
            "builds_and_solves": self.mpc_steps * B,
            "failed": int(self.failed.item()),
            "mean_iters": float(self.iters_total.item()) / solves,
        }


# ---------------------------------------------------------------------------
# LIPM walking controller
# ---------------------------------------------------------------------------
MAX_ZMP_DIST = 100.0  # examples/lipm_walking_controller.py:29


class LIPMWalkingLoop:
    """``B`` walkers running the model-predictive part of the LIPM walking controller in lock step.

    Batched counterpart of examples/lipm_walking_controller.py:304-333. Per MPC period every walker
    (1) rebuilds the ZMP bounds ``e_k`` of its receding horizon from its footstep phase and its goal
    state (``PhaseStepper.get_nb_steps`` + ``update_goal_and_constraints``, :134-213) -- a per-step
    *list* of inequality vectors in the reference, a ``[B, N, 2]`` operand here --, (2) solves its MPC
    problem (triple integrator, nx=3, nu=1, N=16, ZMP rows ``C``; one fused launch for the batch,
    replacing ``solve_mpc`` at :309), (3) integrates the first jerk exactly for ``substeps``
    sub-steps (:216-236, :311-312) and (4) advances its phase (:329-332). Walkers differ by initial
    phase, support foot, stride lengths and foot size; the model (A, B, C) is shared (stride 0).
    Everything stays on the device; the host only enqueues work.

    HIP graphs: ``step`` is not a call to capture once and replay. The host decides per period what it enqueues -- the
    first period also writes the problem of the current phase, a warm start is switched on after it --, and with
    ``fused=False`` the phase and the states are NEW tensors every period, which a captured period would not follow.
    """

    def __init__(self, batch: int, strides=None, foot_size=None, index=None, stride_index=None, support=None,
                 state=None, com_height: float = 0.84, dsp_duration: float = 0.1, ssp_duration: float = 0.7,
                 gravity: float = 9.81, init_support_foot_pos: float = 0.09, nb_timesteps: int = 16,
                 sampling_period: float = 0.1, substeps: int = 15, max_iter: Optional[int] = None,
                 warm_start=False, shared_model: bool = False, flags: int = 0):
        import torch

        _capi.require_gpu()
        dev, f64 = torch.device("cuda", torch.cuda.current_device()), torch.float64
        T, N = float(sampling_period), int(nb_timesteps)
        self.nb_timesteps, self.sampling_period, self.substeps = N, T, int(substeps)
        # flags: MpcqpSolveOpts.flags of every period's solve (_capi.OPT_*), e.g. OPT_ON_CHIP_32 at 17 <= nb_timesteps <= 32
        opt_kw = {"flags": int(flags)} if flags else {}
        self.nb_dsp, self.nb_ssp = int(round(dsp_duration / T)), int(round(ssp_duration / T))
        if 2 * (self.nb_dsp + self.nb_ssp) < N:  # PhaseStepper.__init__, :107-110
            from .exceptions import ProblemDefinitionError

            raise ProblemDefinitionError("there are more than two steps in the receding horizon")
        self.omega = float(np.sqrt(gravity / com_height))

        def dev_t(v, default, dtype, shape):
            a = np.broadcast_to(np.asarray(default if v is None else v), shape)
            return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev)

        self.strides = dev_t(strides, (-0.18, 0.18), f64, (batch, 2))
        self.foot_size = dev_t(foot_size, 0.065, f64, (batch,))
        self.index = dev_t(index, 5, torch.int64, (batch,))  # initial index of the reference, :117
        self.stride_index = dev_t(stride_index, 0, torch.int64, (batch,))
        self.support = dev_t(support, init_support_foot_pos, f64, (batch,))
        if state is None:  # ZMP at the centre of the first foothold, DCM halfway (:300-302)
            s0 = self.support
            state = torch.stack([torch.zeros_like(s0), 0.5 * self.omega * s0, -self.omega**2 * s0], dim=1)
        self.states = dev_t(state.cpu().numpy() if hasattr(state, "cpu") else state, None, f64, (batch, 3))
        # build_mpc_problem (:59-101): shared LTI model, per-walker e / x0 / goal
        A = np.array([[1.0, T, T**2 / 2.0], [0.0, 1.0, T], [0.0, 0.0, 1.0]])
        Bm = np.array([T**3 / 6.0, T**2 / 2.0, T]).reshape((3, 1))
        zmp = np.array([1.0, 0.0, -1.0 / self.omega**2])
        self.zmp_from_state = torch.tensor(zmp, dtype=f64, device=dev)
        Cm = np.array([+zmp, -zmp])
        e0 = np.full((batch, N, 2), MAX_ZMP_DIST)
        self.problem = BatchMPCProblem(A, Bm, Cm, None, e0, N, 1.0, None, 1e-3, np.zeros((batch, 3)),
                                       goal_state=np.zeros((batch, 3)))
        # warm_start: every period begins from the previous period's active set and operator (the model
        # A, B, C is time-invariant here, only the bounds e, x0 and the goal move; MpcqpSolveOpts.warm_state)
        # warm_start="active_set": only last period's active ROWS are kept and enter first, moved one step down the horizon
        # (MPCQP_WARM_ACTIVE_SET with warm_shift = mk = 2: row (k, i) of the last period is row (k - 1, i) of this one)
        self.warm_state = WarmState(self.problem) if warm_start else None
        self._warm_mode = warm_start
        self.model = None
        if shared_model:
            # The matrices never change here, only e / x0 / goal do: factor them ONCE (the reference's own usage of
            # MPCQP, mpc_qp.py:129-163: build, then update_cost_vector / update_constraint_vector per period) and give
            # every period's solve its bounds (mpcqp_solve_model_bounds_batch: up to 32 timesteps). Same plans as the
            # rebuilding loop.
            from .batch import SharedModel

            if warm_start:
                raise ValueError("LIPMWalkingLoop: warm_start and shared_model are exclusive")
            self.model = SharedModel(self.problem)
            self.solver = self.model.prepare(self.problem, max_iter=max_iter, **opt_kw)
        else:
            self.solver = (PreparedSolve(self.problem, max_iter=max_iter, warm_state=self.warm_state, **opt_kw) if warm_start
                           else PreparedSolve(self.problem, max_iter=max_iter, **opt_kw))
        self._k = torch.arange(N, device=dev)
        self._problem_written = False  # e / goal / x0 of the CURRENT phase are in the problem buffers
        self.mpc_steps = 0
        self._stats = torch.zeros((2,), dtype=torch.int64, device=dev)  # [failed, sum of iterations], mpcqp_accumulate_stats
        self.failed, self.iters_total = self._stats[0], self._stats[1]

    # -- PhaseStepper.get_nb_steps (:134-165), vectorised over the batch ---------------------------
    def _segment_counts(self):
        import torch

        nb_dsp, nb_ssp, N = self.nb_dsp, self.nb_ssp, self.nb_timesteps
        zero = torch.zeros_like(self.index)
        offset = self.index
        init_dsp = torch.clamp(nb_dsp - offset, min=0)
        offset = torch.clamp(offset - nb_dsp, min=0)
        init_ssp = torch.clamp(nb_ssp - offset, min=0)
        remaining = N - init_dsp - init_ssp
        next_dsp = torch.clamp(remaining, max=nb_dsp)
        remaining = torch.maximum(zero, remaining - nb_dsp)
        next_ssp = torch.clamp(remaining, max=nb_ssp)
        remaining = torch.maximum(zero, remaining - nb_ssp)
        last_dsp = torch.clamp(remaining, max=nb_dsp)
        remaining = torch.maximum(zero, remaining - nb_dsp)
        last_ssp = torch.clamp(remaining, max=nb_ssp)
        return torch.stack([init_dsp, init_ssp, next_dsp, next_ssp, last_dsp, last_ssp], dim=1)

    def _foot_positions(self):
        nxt = self.support + self.strides.gather(1, self.stride_index[:, None])[:, 0]  # get_next_foot_pos
        last = nxt + self.strides.gather(1, ((self.stride_index + 1) % 2)[:, None])[:, 0]  # get_last_foot_pos
        return nxt, last

    def _write_goal_and_constraints(self) -> None:
        """update_goal_and_constraints (:179-213) for every walker, in place."""
        import torch

        counts = self._segment_counts()  # [B, 6]
        nxt, last = self._foot_positions()
        half = 0.5 * self.foot_size
        free = torch.full_like(self.support, MAX_ZMP_DIST)
        upper = torch.stack([free, self.support + half, free, nxt + half, free, last + half], dim=1)
        lower = torch.stack([free, -(self.support - half), free, -(nxt - half), free, -(last - half)], dim=1)
        ends = torch.cumsum(counts, dim=1)  # step k lies in segment #(ends <= k)
        seg = (self._k[None, :, None] >= ends[:, None, :]).sum(dim=2).clamp(max=5)  # [B, N]
        e = self.problem.e.view(-1, self.nb_timesteps, 2)
        e[:, :, 0] = upper.gather(1, seg)
        e[:, :, 1] = lower.gather(1, seg)
        goal = self.problem.goal_state
        goal.zero_()
        goal[:, 0] = torch.where(counts[:, 4] > 0, last, nxt)
        self.problem.initial_state.copy_(self.states)

    def _integrate(self, jerk):
        """Constant-jerk plant (:216-236), ``substeps`` exact sub-steps like the example (:311-312)."""
        import torch

        dt = self.sampling_period / self.substeps
        p, v, a = self.states[:, 0], self.states[:, 1], self.states[:, 2]
        for _ in range(self.substeps):
            p, v, a = (p + dt * (v + dt * (a / 2 + dt * jerk / 6)), v + dt * (a + dt * (jerk / 2)), a + dt * jerk)
        self.states = torch.stack([p, v, a], dim=1)

    def _advance_phase(self) -> None:
        """phase.advance(); on wrap-around the swing foot becomes the support foot (:329-332)."""
        import torch

        nxt, _ = self._foot_positions()
        index = self.index + 1
        index = torch.where(index >= self.nb_dsp + self.nb_ssp, torch.zeros_like(index), index)
        wrapped = index == 0
        self.support = torch.where(wrapped, nxt, self.support)
        self.stride_index = torch.where(wrapped, (self.stride_index + 1) % 2, self.stride_index)
        self.index = index

    def _advance_fused(self, first: bool) -> None:
        """One launch of ``mpcqp_lipm_advance_stats_batch``: plant + phase + next problem + bookkeeping (for the
        very first period only the problem of the current phase)."""
        p = self.problem
        rc = _capi.load().mpcqp_lipm_advance_stats_batch(
            _dtype_code(p.dtype), self.states.data_ptr(), None if first else self.solver.U.data_ptr(), p.nb_variables,
            None if first else self.solver.status.data_ptr(), None if first else self.solver.iters.data_ptr(),
            None if first else self._stats.data_ptr(), self.nb_timesteps, self.sampling_period, self.substeps,
            self.nb_dsp, self.nb_ssp, MAX_ZMP_DIST, self.index.data_ptr(), self.stride_index.data_ptr(),
            self.support.data_ptr(), self.strides.data_ptr(), self.foot_size.data_ptr(), p.initial_state.data_ptr(),
            p.goal_state.data_ptr(), p.e.data_ptr(), p.batch_size, _stream_ptr())
        _capi.check(rc, "mpcqp_lipm_advance_stats_batch")

    def step(self, nb_mpc_steps: int = 1, fused: bool = True):
        """Advance every walker by ``nb_mpc_steps`` MPC periods: per period one solver launch and one
        fused plant + phase + next-problem launch. ``fused=False`` does the same bookkeeping with torch
        ops (dozens of small launches; kept as a cross-check of the kernel). Asynchronous."""
        import torch

        for _ in range(nb_mpc_steps):
            if fused:
                if not self._problem_written:
                    self._advance_fused(first=True)
                self.solver.launch()
                if self.warm_state is not None and self.mpc_steps == 0:
                    self.solver.set_warm_start(self._warm_mode, warm_shift=2)  # from the second period on
                self._advance_fused(first=False)
                self._problem_written = True
            else:
                self._problem_written = False
                self._write_goal_and_constraints()
                self.solver.launch()
                if self.warm_state is not None and self.mpc_steps == 0:
                    self.solver.set_warm_start(self._warm_mode, warm_shift=2)
                ok = self.solver.status == 0
                jerk = torch.where(ok, self.solver.U[:, 0], torch.zeros_like(self.solver.U[:, 0]))
                self._integrate(jerk)
                self._advance_phase()
                _capi.load().mpcqp_accumulate_stats(self.solver.status.data_ptr(), self.solver.iters.data_ptr(),
                                                    self.problem.batch_size, self._stats.data_ptr(), _stream_ptr())
            self.mpc_steps += 1
        return self.states

    def zmp(self):
        """Current ZMP of every walker (``zmp_from_state``, :53-55)."""
        return self.states @ self.zmp_from_state

    def stats(self) -> Dict[str, float]:
        B = self.problem.batch_size
        solves = max(self.mpc_steps * B, 1)
        return {"loops": B, "mpc_steps": self.mpc_steps, "builds_and_solves": self.mpc_steps * B,
                "failed": int(self.failed.item()), "mean_iters": float(self.iters_total.item()) / solves}


# ---------------------------------------------------------------------------
# Closed loops of any shared model (mpcqp_model_periods_batch)
# ---------------------------------------------------------------------------
class ModelClosedLoop:
    """``B`` independent control loops of one :class:`SharedModel` against a linear plant, advancing in lock step.

    Per period every loop solves the model's problem at its state, applies the first input of the plan (zero when no plan
    was found -- the loop carries on and the period is counted in ``failed``) and steps its plant
    ``x+ = Ap x + Bp u0 + d``: the rules of :class:`WIPClosedLoop`, with the plant given as data. ``plant=(Ap, Bp)`` is
    ``[nx, nx]`` / ``[nx, nu]`` shared or ``[B, nx, nx]`` / ``[B, nx, nu]`` per loop and defaults to the model's own A, B.
    ``goal`` (``[nx]``, ``[B, nx]``), ``targets`` (``[N nx]``, ``[B, N nx]``) and ``disturbance`` (``[nx]``, ``[B, nx]``) are
    constant, or carry a period axis in front of the last one (``[B|1, P, nx]``, ``[B|1, P, N nx]``): the loop keeps a period
    counter and ``step`` reads on from where the last call stopped.

    ``step(n, fused=True)`` runs the ``n`` periods in ONE launch (``mpcqp_model_periods_batch``: float64, N nu <= 16,
    1 <= N mk <= 32, nx <= 16, the model's own bounds; ``BackendError`` outside that envelope). ``fused=False`` is the loop
    written by hand -- a :class:`PreparedModelSolve` launch plus the plant step in torch per period -- and serves everything
    ``SharedModel`` solves. ``warm=True`` (fused only: ``step(fused=False)`` then raises ``ValueError``) starts every period of a launch but the first from the active set
    and operator of the period before, kept in registers; a warm period that does not end verified-solved is solved again
    cold (``stats()["resolved_cold"]``), so the trajectories are those of the cold loop to rounding.

    ``feas_tol`` defaults to 1e-9 here, not to the solvers' 1e-12, on purpose: a state-constrained loop whose plant is its
    model lands exactly ON a bound, and the next period's row on x_0 -- which no input can move -- is then satisfied only to
    rounding. With the C oracle on the triple-integrator family (e = 3, 67 loops, 7 periods) an error of 1e-11 on the
    acceleration turned 330 of 469 periods INFEASIBLE under ``1e-12 (1 + |h|)`` and none at 1e-9, where the trajectories
    moved by 2e-11.

    Measured (profiles/model_loop.md, tools/bench_model_loop.py: triple-integrator family, 50 periods, one MI355X, us per
    period for the whole batch, by hand / fused cold / fused warm): B = 256: 91 / 11.0 / 6.1; 1024: 87 / 11.4 / 6.7;
    4096: 88 / 16.9 / 12.9; 65536: 174 / 159 / 131. The fused launch wins at every size measured -- by 5-8x up to 4096,
    where the loop by hand is bound by the HOST (about 87 us per period of enqueueing, whatever B: the ratio measures that
    cost, not one kernel against another), by 1.10x (cold) where the device is the bound.
    The warm start took 0.40 of the cold iterations there; on loops whose active set does not carry over (input boxes
    with a mismatched plant) it took MORE iterations than cold. Nothing is switched here by a threshold."""

    def __init__(self, model: SharedModel, x0, goal=None, targets=None, plant=None, disturbance=None, warm: bool = False,
                 feas_tol: float = 1e-9, max_iter: Optional[int] = None, record: bool = True):
        import torch

        t = model.template
        self.model = model
        self._dev, self._dt = t.device, t.dtype
        self.nx, self.nu, self.N = t.state_dim, t.input_dim, t.nb_timesteps
        self.n, self.m = t.nb_variables, t.nb_constraints
        as_t = lambda a: None if a is None else torch.as_tensor(a, dtype=self._dt, device=self._dev).contiguous()  # noqa: E731
        self.states = as_t(np.asarray(x0, dtype=float) if not torch.is_tensor(x0) else x0).clone()
        if self.states.ndim != 2 or self.states.shape[1] != self.nx:
            raise ValueError(f"x0 must be [B, {self.nx}]")
        B = self.batch = self.states.shape[0]
        self._goal = self._reference(as_t(goal), self.nx, "goal")
        self._targets = self._reference(as_t(targets), self.N * self.nx, "targets")
        self._dist = self._reference(as_t(disturbance), self.nx, "disturbance")
        Ap, Bp = (t.A[0, 0], t.B[0, 0]) if plant is None else plant
        self._Ap, self._Bp = as_t(Ap).clone(), as_t(Bp).clone()
        if self._Ap.shape[-2:] != (self.nx, self.nx) or self._Bp.shape[-2:] != (self.nx, self.nu):
            raise ValueError("plant must be (Ap [nx, nx] or [B, nx, nx], Bp [nx, nu] or [B, nx, nu])")
        for M in (self._Ap, self._Bp):
            if M.ndim == 3 and M.shape[0] != B:
                raise ValueError("a per-loop plant needs one matrix per loop")
        self.warm, self.record = bool(warm), bool(record)
        self._feas_tol, self._max_iter = float(feas_tol), max_iter
        self._opts = _opts_for_loop(max_iter, feas_tol)
        self.periods = 0
        self._loopstats = torch.zeros((B, 3), dtype=torch.int64, device=self._dev)
        self.U = torch.zeros((B, self.n), dtype=self._dt, device=self._dev)
        self.lam = torch.zeros((B, max(self.m, 1)), dtype=self._dt, device=self._dev)
        self.status = torch.zeros((B,), dtype=torch.int32, device=self._dev)
        self.iters = torch.zeros((B,), dtype=torch.int32, device=self._dev)
        self._X, self._U0 = [self.states.clone()[:, None]], []
        self._solver = None  # fused=False: a PreparedModelSolve on buffers of its own, built on first use

    # ------------------------------------------------------------------ references
    def _reference(self, a, width: int, what: str):
        """(tensor, batch_stride, period_stride, periods or None) of a reference that is constant or has a period axis."""
        if a is None:
            return None
        if a.shape[-1] != width or a.ndim > 3:
            raise ValueError(f"{what}: last axis must be {width}, with at most a loop and a period axis in front")
        if a.ndim == 3:  # [B|1, P, width]
            if a.shape[0] not in (1, self.batch):
                raise ValueError(f"{what}: first axis must be 1 or the number of loops")
            return a, (a.shape[1] * width if a.shape[0] != 1 or self.batch == 1 else 0), width, a.shape[1]
        if a.ndim == 2 and a.shape[0] not in (1, self.batch):
            raise ValueError(f"{what}: first axis must be 1 or the number of loops")
        return a, (width if a.ndim == 2 and (a.shape[0] != 1 or self.batch == 1) else 0), 0, None

    def _operand(self, ref, t: int):
        if ref is None:
            return _capi.Operand(None, 0, 0)
        a, bs, ps, _ = ref
        return _capi.Operand(a.data_ptr() + t * ps * a.element_size(), bs, ps)

    def _at(self, ref, t: int):
        """The reference of period t as a tensor that broadcasts against [B, width]."""
        a, _, ps, _ = ref
        return a[:, t] if ps else a

    def _check_periods(self, n: int) -> None:
        for ref, what in ((self._goal, "goal"), (self._targets, "targets"), (self._dist, "disturbance")):
            if ref is not None and ref[3] is not None and self.periods + n > ref[3]:
                raise ValueError(f"{what} is laid out for {ref[3]} periods; {self.periods} have run and {n} more were asked for")

    # ------------------------------------------------------------------ stepping
    def step(self, nb_periods: int = 1, fused: bool = True):
        """Advance every loop by ``nb_periods`` periods. Asynchronous; returns ``self.states``."""
        n = int(nb_periods)
        if n < 1:
            raise ValueError("nb_periods must be at least 1")
        self._check_periods(n)
        if fused:
            self._step_fused(n)
        else:
            if self.warm:
                raise ValueError("warm=True is carried inside a fused launch only; step(fused=False) always starts cold")
            for _ in range(n):
                self._step_by_hand()
        return self.states

    def _step_fused(self, n: int) -> None:
        import torch

        if self._dt != torch.float64 or self.n > 16 or not (1 <= self.m <= 32) or self.nx > 16 or self.model.per_problem_bounds:
            raise BackendError(
                "ModelClosedLoop.step(fused=True) serves float64 models with N nu <= 16, 1 <= N mk <= 32, nx <= 16 and "
                f"the model's own bounds (mpcqp_model_periods_batch); this one has N nu = {self.n}, N mk = {self.m}, "
                f"nx = {self.nx}, {self._dt}" + (", bounds per problem" if self.model.per_problem_bounds else "")
                + ". step(fused=False) serves everything SharedModel solves.", code=_capi.EUNSUPPORTED)
        t = self.periods
        B = self.batch
        plant = _capi.LoopPlant(
            _capi.Operand(self._Ap.data_ptr(), self.nx * self.nx if self._Ap.ndim == 3 else 0, 0),
            _capi.Operand(self._Bp.data_ptr(), self.nx * self.nu if self._Bp.ndim == 3 else 0, 0),
            self._operand(self._dist, t))
        goal, targets = self._operand(self._goal, t), self._operand(self._targets, t)
        X = U0 = None
        if self.record:
            X = torch.empty((B, n + 1, self.nx), dtype=self._dt, device=self._dev)
            U0 = torch.empty((B, n, self.nu), dtype=self._dt, device=self._dev)
        out = _capi.LoopOut(None if X is None else X.data_ptr(), None if U0 is None else U0.data_ptr(),
                            self._loopstats.data_ptr())
        rc = _capi.load().mpcqp_model_periods_batch(
            C.byref(self.model.dims), self.model.model.data_ptr(), C.byref(plant), self.states.data_ptr(), C.byref(goal),
            C.byref(targets), B, n, int(self.warm), C.byref(self._opts), self.U.data_ptr(),
            self.lam.data_ptr() if self.m else None, self.status.data_ptr(), self.iters.data_ptr(), C.byref(out), _stream_ptr())
        _capi.check(rc, "mpcqp_model_periods_batch")
        self.periods += n
        if self.record:
            self._X.append(X[:, 1:])
            self._U0.append(U0)

    def _step_by_hand(self) -> None:
        """One period as users wrote it before: a PreparedModelSolve launch, then the plant step in torch."""
        import torch

        t = self.periods
        if self._solver is None:
            B = self.batch
            x0 = self.states.clone()
            goal = None if self._goal is None else torch.zeros((B, self.nx), dtype=self._dt, device=self._dev)
            tg = None if self._targets is None else torch.zeros((B, self.N * self.nx), dtype=self._dt, device=self._dev)
            self._solver = self.model.prepare(self.model.problem_for(x0, goal, tg), return_multipliers=True,
                                              max_iter=self._max_iter, feas_tol=self._feas_tol)
        s = self._solver
        p = s.problem
        p.initial_state.copy_(self.states)
        if self._goal is not None:
            p.goal_state.copy_(self._at(self._goal, t).expand_as(p.goal_state))
        if self._targets is not None:
            p.target_states.copy_(self._at(self._targets, t).expand_as(p.target_states))
        s.launch()
        ok = (s.status == 0)[:, None]
        u0 = torch.where(ok, s.U[:, :self.nu], torch.zeros((), dtype=self._dt, device=self._dev))
        if self._Ap.ndim == 3:
            x = torch.bmm(self._Ap, self.states[:, :, None])[:, :, 0]
        else:
            x = self.states @ self._Ap.T
        if self._Bp.ndim == 3:
            x = x + torch.bmm(self._Bp, u0[:, :, None])[:, :, 0]
        else:
            x = x + u0 @ self._Bp.T
        if self._dist is not None:
            x = x + self._at(self._dist, t)
        self.states.copy_(x)
        self._loopstats[:, 0] += s.status != 0
        self._loopstats[:, 1] += s.iters
        # (the last period's plan is the prepared solve's own output: no copies)
        self.U, self.status, self.iters = s.U, s.status, s.iters
        if self.m:
            self.lam = s.lam
        self.periods += 1
        if self.record:
            self._X.append(self.states.clone()[:, None])
            self._U0.append(u0[:, None])

    # ------------------------------------------------------------------ results
    @property
    def X(self):
        """[B, periods + 1, nx]: the state before every period and after the last (``record=True``)."""
        import torch

        return torch.cat(self._X, dim=1)

    @property
    def U0(self):
        """[B, periods, nu]: the input applied in every period (``record=True``)."""
        import torch

        if not self._U0:
            return torch.empty((self.batch, 0, self.nu), dtype=self._dt, device=self._dev)
        return torch.cat(self._U0, dim=1)

    @property
    def plan(self):
        """The LAST period's plan (``BatchPlan``: U, status, iters, multipliers) at the state before that period."""
        from .batch import BatchPlan

        x_before = self.X[:, -2] if self.record and self.periods else self.states
        return BatchPlan(self.model.problem_for(x_before), self.U, self.status, self.iters, self.lam if self.m else None)

    @property
    def failed(self):
        """0-d int64 device tensor: periods of any loop without a plan (the zero input was applied)."""
        return self._loopstats[:, 0].sum()

    @property
    def iters_total(self):
        """0-d int64 device tensor: active-set iterations of all periods so far."""
        return self._loopstats[:, 1].sum()

    def stats(self) -> Dict[str, float]:
        solves = max(self.periods * self.batch, 1)
        return {
            "loops": self.batch,
            "periods": self.periods,
            "failed": int(self.failed.item()),
            "mean_iters": float(self.iters_total.item()) / solves,
            "resolved_cold": int(self._loopstats[:, 2].sum().item()),
        }


def _opts_for_loop(max_iter, feas_tol):
    from .batch import _opts

    return _opts(max_iter, feas_tol)
