#!/usr/bin/env python3
"""A Monte-Carlo closed loop of the triple integrator (the model of examples/triple_integrator.py) through ModelClosedLoop.

4096 loops start from random states and are driven to their goals for 50 control periods against a plant whose input
gain is up to 10 % weaker than the model's, per loop, under a constant disturbance on position and velocity. (A stronger
gain would carry a loop that rides the acceleration bound past it, and the row on x_0 -- which no input can move --
would make every later period infeasible.) The 50 periods are ONE launch (``mpcqp_model_periods_batch``); the same loop
written by hand -- a shared-model solve plus a torch plant step per period -- runs next to it for comparison.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout

import numpy as np
import torch

from qpmpc_amd import BatchMPCProblem, ModelClosedLoop, SharedModel
from qpmpc_amd import workloads as W

N, B, PERIODS = 16, 4096, 50
A, Bm, C, e = W.triple_integrator_matrices(N)
rng = np.random.default_rng(0)
x0 = np.stack([rng.uniform(-.5, .5, B), rng.uniform(-.5, .5, B), rng.uniform(-2.5, 2.5, B)], 1)
goal = np.stack([rng.uniform(.5, 1.5, B), np.zeros(B), np.zeros(B)], 1)
Bp = Bm[None] * rng.uniform(0.9, 1.0, (B, 1, 1))  # every loop's plant has an input gain of its own
dist = np.zeros((B, 3))
dist[:, :2] = 1e-3 * rng.standard_normal((B, 2))

# the model is factored once: everything that does not depend on the state
model = SharedModel(BatchMPCProblem(A, Bm, C, None, e, N, 1.0, None, 1e-6, np.zeros((1, 3)), goal_state=np.zeros((1, 3))))

for name, kw in (("fused, cold", dict(warm=False)), ("fused, warm start", dict(warm=True))):
    loop = ModelClosedLoop(model, x0, goal=goal, plant=(A, Bp), disturbance=dist, **kw)
    loop.step(PERIODS)  # one launch
    torch.cuda.synchronize()
    miss = (loop.states[:, 0].cpu() - torch.tensor(goal[:, 0])).abs()
    print(f"{name:18s}: {loop.stats()}, |position - goal| mean {miss.mean():.2e} max {miss.max():.2e}, "
          f"peak |acceleration| {loop.X[:, :, 2].abs().max():.3f} (bound 3)")

by_hand = ModelClosedLoop(model, x0, goal=goal, plant=(A, Bp), disturbance=dist)
by_hand.step(PERIODS, fused=False)  # a solve launch and a torch plant step per period
torch.cuda.synchronize()
print("by hand           :", by_hand.stats(), "max |X - X_fused| = %.2e" % float((by_hand.X - loop.X).abs().max()))
