"""CPU test (no GPU): every launch the library refused on the host when tests/golden/refusal_codes.npz was recorded
(tools/gen_golden_refusals.py) is still refused, with the same code -- through the five forward exports themselves
(mpcqp_build_solve_batch, mpcqp_stagewise_solve_batch, mpcqp_solve_model_batch, mpcqp_solve_model_bounds_batch,
mpcqp_solve_batch), in both dtypes, with every flag alone and next to MPCQP_OPT_ON_CHIP_32 / MPCQP_OPT_FOUR_PER_WAVE, with
and without a pairing order, a warm state of each warm_start mode, a workspace, the bounds, at the edges of every kernel's
envelope. Where two rules refuse one launch the code returned says which is checked first, so the order of the checks is
pinned with the rules. The pairs of rules that overlap on the grid, per export (the first of a pair wins):

mpcqp_build_solve_batch
  a missing argument (EINVAL) / every rule below (the rows without bounds)
  order not served (EUNSUPPORTED) / FOUR_PER_WAVE refused by name, the ON_CHIP_32 envelope and mask, warm state without
    a record, WARM_ACTIVE_SET against the record kind, PIPELINE_FACTOR outside the narrow path (all EUNSUPPORTED), short
    warm state (EWORKSPACE), no kernel (ETOOLARGE: (4, 10, 26, 1), n = 260 with nu = 10), short workspace (EWORKSPACE)
  FOUR_PER_WAVE by name / the ON_CHIP_32 mask (the flag pair), warm-state rules, PIPELINE_FACTOR, short workspace
  ON_CHIP_32 envelope and mask / warm-state rules, PIPELINE_FACTOR, short warm state, short workspace
  warm state without a record or of the wrong kind, PIPELINE_FACTOR (EUNSUPPORTED) / short warm state (EWORKSPACE)
  short warm state (EWORKSPACE) / warm state next to FORCE_LDS or ONE_PER_WAVE at the pair kernel's sizes
    (EUNSUPPORTED: refused last, so the short record answers EWORKSPACE), short workspace
  float32 solved in float64: the copies' workspace (EWORKSPACE) / every rule after the ON_CHIP_32 one (they are checked
    by the float64 launch)
mpcqp_stagewise_solve_batch
  no stage-wise kernel for the system (EUNSUPPORTED: nx = 20, the shapes with nu = 10, no rows) / an order, a warm state
    (EUNSUPPORTED), short workspace (EWORKSPACE)
  order (EUNSUPPORTED) / warm state (EUNSUPPORTED) / short workspace (EWORKSPACE)
mpcqp_solve_model_batch, mpcqp_solve_model_bounds_batch
  warm state / order outside the pair kernel's model mode / FOUR_PER_WAVE by name / bounds per problem past the
    on-chip kernels, ON_CHIP_32 outside its envelope or next to another choice (all EUNSUPPORTED) / the workgroup kernel's
    LDS (ETOOLARGE: n = 33 with m = 33 still fits; (4, 10, 8, 2), n = 80, does not)
  FOUR_PER_WAVE by name (EUNSUPPORTED) / bounds per problem without rows (EINVAL: (3, 1, 8, 0))
mpcqp_solve_batch
  order / warm state / ON_CHIP_32 envelope, dtype and mask (all EUNSUPPORTED) / n > 256 (ETOOLARGE) / short workspace
    (EWORKSPACE)

The replay runs in a process of its own that hides every device from the runtime before the library is loaded: the
pointers it hands over are placeholders, and a launch that a change wrongly serves must fail in the runtime, not run."""
import os
import subprocess
import sys

import numpy as np

from golden_util import GOLDEN

import tools.gen_golden_refusals as gen


def test_refused_launches_keep_their_codes(tmp_path):
    golden = os.path.join(GOLDEN, "refusal_codes.npz")
    want = np.load(golden)["codes"]
    rows = gen.grid()
    assert want.shape == (len(rows),)
    out = str(tmp_path / "codes.npy")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")  # (the script hides them as well)
    subprocess.run([sys.executable, gen.__file__, "--replay", golden, out], check=True, timeout=120, env=env)
    got = np.load(out)
    rows, want = rows[want < 0], want[want < 0]
    assert len(want) > 300000 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    names = ("export", "dtype", "nx", "nu", "N", "mk", "flags", "order", "warm", "roomy", "e")
    report = [f"{gen.EXPORTS[rows[i][0]]} {dict(zip(names[1:], rows[i][1:].tolist()))}: got {got[i]}, recorded {want[i]}" for i in bad[:20]]
    assert len(bad) == 0, f"{len(bad)} refused launches changed their code:\n" + "\n".join(report)
