"""The crowd step form (worlds of 17..64 agents) against the float64 oracle OFF the configuration every other crowd test runs in (table
actions, the default table, plain unicycle dynamics, default numbers).  `crowd_tile` has its own copies of the action decode (clamp,
table in LDS), of all three dynamics, of the K-step prefetch of continuous actions and of every reward / termination statement, and
`generate_world_v2` takes the agent count at run time: here every numeric `cavoid_cfg` field is off its default on both sides, actions
are continuous for all three dynamics, the table has 5 / 11-wide / 32 entries with out-of-range indices, and a one-step time budget
restarts every world at every step.

The cases come from tests/cfg_regimes.py; tests/test_cfg_regimes_host.py proves on the CPU that each case sees what it is about.  The bar
is tests/test_gpu_parity.py's `_compare_step` (cfg_regimes.drive_gpu): flags, float32 state and is_learning / num_other exact, float64
state <= 1e-9 (<= 1e-12 after the reset), observations and rewards <= 1e-5 with the heading on the circle, the episode counters equal
after every step, and every launch ran the CROWD form.  Shapes, the smallest at which the lane mapping differs: 17 x 50 (three worlds
per wavefront, ragged last one), 24 x 65 (two), 33 x 33 (one, 31 idle lanes), 64 x 20 (all lanes)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import cfg_regimes as R
from tests.gpu_support import _env

pytestmark = pytest.mark.gpu

CROWD = ("CROWD", 0)


def _drive(cid):
    case = R.BY_ID[cid]
    assert 17 <= case.N <= 64
    env = _env(case.W, case.N, seed=case.seed, **case.over)
    run = R.drive_gpu(case, env, "CROWD", CROWD)
    R.assert_events(case, run)
    return case, env, run


@pytest.mark.parametrize("cid", [c.cid for c in R.select("crowd-clipped-") + R.select("crowd-unclipped-")])
def test_crowd_every_numeric_field_off_its_default(cid):
    """CLIPPED / UNCLIPPED with RING on a pool of 200 and BOX generated inside the step: the reset against the generator, 140 single
    steps, one 20-step launch in slots and one 5-step packed launch"""
    case, env, run = _drive(cid)
    env.close()


@pytest.mark.parametrize("cid", [c.cid for c in R.select("crowd-cont-")])
def test_crowd_continuous_actions_against_the_oracle(cid):
    """continuous actions, all three dynamics: 50 single steps, then K = 16 launches in slots (one shorter than its slots) and packed"""
    case, env, run = _drive(cid)
    if case.over["dynamics"] == 2:          # table actions have no velocity meaning: refused for the holonomic dynamics, loudly
        with pytest.raises(RuntimeError):
            env.step_autoreset(torch.zeros((case.W, case.N), dtype=torch.int32, device="cuda"))
    env.close()


@pytest.mark.parametrize("cid", [c.cid for c in R.select("crowd-max-turn-") + R.select("crowd-table")])
def test_crowd_action_tables_and_out_of_range_indices(cid):
    """the max-turn clamp on the WIDE table, 5 and 32 actions; raw indices carry -1, num_actions, INT32_MIN and INT32_MAX (clamped by
    the kernel, handed to the oracle clamped)"""
    case, env, run = _drive(cid)
    assert env.num_actions == R.num_actions(case)
    env.close()


@pytest.mark.parametrize("cid", [c.cid for c in R.select("crowd-pressure-")])
def test_crowd_restart_pressure(cid):
    """a time budget of one step: every world restarts at about every step, from the pool and from both generators inside the step"""
    case, env, run = _drive(cid)
    assert np.array_equal(env.episode.cpu().numpy().view(np.uint32), run.ep) and run.ep.min() >= 1
    env.close()
