"""The two trims of the relay step -- mirrored pair distances (CAVOID_MIRROR_DIST: a lane computes half of its neighbours' distances
and fetches the rest from the mirror lane, csrc/cavoid_kernels.hpp) and per-role argument loads (CAVOID_RELAY_ROLE_ARGS,
csrc/cavoid_relay.hpp) -- change no bit of any output.

Two checks on the same shapes:
  * the product against `build.build_plain_dist()` (both trims compiled out), run in a child process through CAVOID_LIB: observations,
    rewards, done flags, game_over, state and episode counters equal bit for bit, after the reset and in every step of every launch;
  * the product against the float64 oracle with the project's usual bars (flags exact, observations and rewards 1e-5): a fault common to
    both builds cannot pass.

Shapes: N = 3, 4, 5, 6 agents per world with a ragged last tile (two full tiles and 3 worlds more; 21 worlds at N = 4: one tile and 5),
worlds of 2 .. N agents (absent rows), a time budget that restarts worlds inside every launch.  Launches of K = 12 steps into per-step
slots and packed records, with 2, 3 and 4 observation wavefronts (RELAY), as the two-wavefront pipeline (PIPE) and one step per launch
(STEP: CAVOID_QUAD=0 -- the quad kernel makes one distance per lane and has no mirror).

Where the mirror runs: the K-step forms at every N, and the one-step form up to N = 5.  From N = 6 on the one-step form parks its sort
keys and rolls its pair loop (PARK, cavoid_kernels.hpp): it computes every slot in both builds, so the single steps of the N = 6 cases
and the N = 10 x 13 STEP case hold only that the change left that form alone.  The shared pair pass at an even N with FOUR fetched slots
(N = 10: slots 5 .. 8 through __shfl) runs in the two N = 10 x 13 K-step cases: the pipeline (PIPE) and the plain step loop (LOOP_PF).

One look-ahead case (R = 128, two launches of 64 steps): the top-up wavefront with its own argument loads is still carried -- no refill
launch behind the first fill."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import cfg_regimes as R  # noqa: E402

K = 12
SEED = 19


def _spec(tag, N, W, env, single_form, k_form, plan, **source):
    over = dict(R.CLIPPED, **R.MAX_TURN)
    over.update(R.RING)                                     # gen_min_agents = 2: worlds of 2 .. N agents
    over.update(max_time_ratio=R.TOPUP_RATIO)               # an episode ends every four or five steps
    over.update(source)
    case = R.Case("trim-" + tag, "trim", N, W, SEED, over, {}, plan, "goal", 2, ("restart", "collision"), None, (single_form, k_form))
    return case, dict(env, CAVOID_QUAD="0")


def _specs():
    out = []
    k_plan = (("single", 1, 1),) * 4 + (("slots", K, K), ("packed", K, K))
    for N in (3, 4, 5, 6):
        wpw = 64 // N
        W = 21 if N == 4 else 2 * wpw + 3
        for nc in (2, 3, 4):
            out.append(_spec("n%dx%d-relay%d" % (N, W, nc), N, W, dict(CAVOID_RELAY_CONSUMERS=str(nc)), "STEP", "RELAY", k_plan))
        out.append(_spec("n%dx%d-pipe" % (N, W), N, W, dict(CAVOID_PIPELINE="1"), "STEP", ("PIPE", 0), k_plan))
    out.append(_spec("n10x13-step", 10, 13, {}, "STEP", None, (("single", 1, 1),) * K))
    out.append(_spec("n10x13-pipe", 10, 13, dict(CAVOID_PIPELINE="1"), "STEP", ("PIPE", 0), k_plan))
    out.append(_spec("n10x13-loop", 10, 13, dict(CAVOID_PIPELINE="0"), "STEP", ("LOOP_PF", 0), k_plan))
    out.append(_spec("n4x21-lookahead128", 4, 21, {}, "STEP", "RELAY", (("slots", 64, 64), ("packed", 64, 64)), gen_pool_size=0, gen_lookahead=128))
    return out


SPECS = _specs()
BY_ID = {case.cid: (case, env) for case, env in SPECS}
IDS = [case.cid for case, _ in SPECS]


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _env(case, env):
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = case.N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = case.N - 1
            EnvConfig.__init__(self)
    with _environ(env):                                     # (the launch forms are chosen when the env is created)
        return BatchedCollisionAvoidanceEnv(case.W, Cfg(), device="cuda:0", seed=case.seed, **case.over)


def collect(cid):
    """every output of the case's launches on whatever library this process has loaded, as numpy arrays, and the forms that ran"""
    import torch
    case, envv = BY_ID[cid]
    env = _env(case, envv)
    rng = np.random.default_rng(case.seed + 1)
    out, forms, slots = [env.reset().cpu().numpy()], [], {}
    for kind, k, n in case.plan:
        acts = np.stack([R._goal_seeking_actions(rng, case.W, case.N) for _ in range(k)])
        if kind == "single":
            got = env.step_autoreset(torch.from_numpy(acts[0]).cuda())
        else:
            if kind not in slots:
                slots[kind] = env.new_step_slots(k, packed=(kind == "packed"))
            a = torch.from_numpy(acts).cuda()
            got = env.step_autoreset_packed(a, slots[kind], n_steps=n) if kind == "packed" else env.step_autoreset_n(a, n_steps=n, slots=slots[kind])
        out += [v.cpu().numpy() for v in got]
        forms.append("%s/%d" % env.last_step_form)
        out += [v.cpu().numpy() for v in env.get_state()] + [env.episode.cpu().numpy()]
    info = env.lookahead_info
    env.close()
    return out, forms, info


def _dump(path):
    arrays = {}
    for cid in IDS:
        out, forms, info = collect(cid)
        for k, a in enumerate(out):
            arrays["%s|%03d" % (cid, k)] = a
        arrays["%s|forms" % cid] = np.array(forms)
        arrays["%s|info" % cid] = np.array(info, np.int64)
    np.savez(path, **arrays)


if __name__ == "__main__":                                  # the child process of `plain_build` (CAVOID_LIB: the variant)
    _dump(sys.argv[1])
    print("DUMPED", flush=True)
    sys.exit(0)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain_build(tmp_path_factory):
    """every case once on the variant without the trims, in ONE child process"""
    from rl_collision_avoidance_amd import build
    lib = build.variant_path("plaindist")
    if not os.path.exists(lib):
        if build.shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("no prebuilt plain-distance variant and no hipcc on this box")
        lib = build.build_plain_dist()
    path = str(tmp_path_factory.mktemp("relay_trim") / "plain.npz")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, timeout=600, env=dict(os.environ, CAVOID_LIB=lib),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and "DUMPED" in run.stdout, run.stderr[-3000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _want_forms(case):
    single_form, k_form = case.forms
    return [single_form if kind == "single" else (k_form if isinstance(k_form, str) else k_form[0]) for kind, _, _ in case.plan]


@pytest.mark.parametrize("cid", IDS)
def test_bit_for_bit_the_build_without_the_trims(cid, plain_build):
    case, envv = BY_ID[cid]
    out, forms, info = collect(cid)
    assert [f.split("/")[0] for f in forms] == _want_forms(case), forms
    nc = int(envv.get("CAVOID_RELAY_CONSUMERS", 0))
    if nc:                                                  # (N = 5 with four and the wider packed rows: beyond the 80 KB of LDS, the launcher takes three)
        ran = {int(f.split("/")[1]) for f in forms if f.startswith("RELAY")}
        assert ran == {nc} or (case.N >= 5 and nc == 4 and ran <= {3, 4}), forms
    assert list(plain_build["%s|forms" % cid]) == forms     # both builds ran the same kernels
    assert tuple(plain_build["%s|info" % cid]) == tuple(info)
    names = sorted(k for k in plain_build if k.startswith(cid + "|") and k[-3:].isdigit())
    assert len(names) == len(out)
    for k, (name, a) in enumerate(zip(names, out)):
        b = plain_build[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (cid, k)
        assert a.tobytes() == b.tobytes(), (cid, k, int((a != b).sum()))


@pytest.mark.parametrize("cid", IDS)
def test_the_product_against_the_oracle(cid):
    case, envv = BY_ID[cid]
    env = _env(case, envv)
    run = R.drive_gpu(case, env, *case.forms)
    R.assert_events(case, run)
    if "gen_lookahead" in case.over:
        assert env.lookahead_info[0] == 1, env.lookahead_info    # the first fill and nothing else: every launch carried the top-up
    env.close()


def test_the_shapes_hold_absent_agents_and_ragged_tiles():
    for case, _ in SPECS:
        run = R.OracleRun(case)
        present = (run.st.flags.reshape(case.W, case.N) & R.F_PRESENT) != 0
        assert (~present).any() and (present.sum(axis=1) >= 2).all(), case.cid
        assert case.W % (64 // case.N) != 0, case.cid
