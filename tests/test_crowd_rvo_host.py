"""CPU tests of ORCA agents in crowd worlds (rvo_enabled = 2 = CAVOID_RVO_WAVE, CAVOID_FORM_CROWD_RVO): what cavoid_create accepts and
refuses, what make_cfg picks, the header's declarations, and the built library's six ORCA-carrying crowd kernels (no scratch, the
crowd form's workgroup sizes)."""
import ctypes as C
import os
import re

import pytest

from tests.host_support import LLVM, _cfg, _create, _kernel_notes, _no_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HAVE_LLVM = os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))


def _rvo_cfg(n, value=2):
    cfg = _cfg(n)
    cfg.rvo_enabled = value
    cfg.gen_nonlearning_fraction = 0.5
    cfg.gen_rvo_fraction = 0.5
    return cfg


@pytest.mark.parametrize("n", [17, 20, 33, 64])
def test_create_accepts_wave_orca_in_crowd_worlds(n):
    _no_gpu()
    assert _create(_rvo_cfg(n)) == -5        # CAVOID_ENODEVICE: the configuration passed, only the device is missing


def test_create_refuses_wave_orca_at_exactly_16_agents():
    _no_gpu()
    assert _create(_rvo_cfg(16)) == -4       # the tile forms' line scratch ends at 15, the crowd form starts at 17
    cfg = _rvo_cfg(17)                       # ... what a user of 16 agents takes instead
    cfg.gen_min_agents, cfg.gen_max_agents = 2, 16
    assert _create(cfg) == -5


def test_up_to_15_agents_any_non_zero_value_is_the_tile_forms_orca():
    _no_gpu()
    for n in (2, 10, 15):
        assert _create(_rvo_cfg(n, 1)) == -5 and _create(_rvo_cfg(n, 2)) == -5


def test_lane_orca_and_the_look_ahead_stay_refused_in_crowd_worlds():
    _no_gpu()
    assert _create(_rvo_cfg(20, 1)) == -4
    cfg = _rvo_cfg(20)
    cfg.gen_pool_size = 0
    cfg.gen_lookahead = 8
    assert _create(cfg) == -4
    cfg = _cfg(20)                           # RVO agents generated but no ORCA in the step: a bad configuration, as at every size
    cfg.gen_nonlearning_fraction = 0.5
    cfg.gen_rvo_fraction = 0.5
    assert _create(cfg) == -1


def test_make_cfg_picks_the_form_by_agent_count():
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.batched_env import make_cfg
    from rl_collision_avoidance_amd.config import EnvConfig

    def cfg_of(n, scripted, rvo):
        class Cfg(EnvConfig):
            def __init__(self):
                self.MAX_NUM_AGENTS_IN_ENVIRONMENT = n
                self.SCRIPTED_AGENT_FRACTION = scripted
                self.SCRIPTED_RVO_FRACTION = rvo
                EnvConfig.__init__(self)
        return make_cfg(Cfg())
    assert cfg_of(20, 0.5, 0.33).rvo_enabled == 2 == _lib.RVO_WAVE
    assert cfg_of(64, 0.5, 1.0).rvo_enabled == 2
    assert cfg_of(10, 0.5, 0.33).rvo_enabled == 1
    assert cfg_of(16, 0.5, 0.33).rvo_enabled == 1
    assert cfg_of(20, 0.0, 0.33).rvo_enabled == 0 and cfg_of(20, 0.5, 0.0).rvo_enabled == 0
    class Cfg20(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = 20
            self.SCRIPTED_AGENT_FRACTION = 0.5
            self.SCRIPTED_RVO_FRACTION = 0.33
            EnvConfig.__init__(self)
    assert make_cfg(Cfg20(), rvo_enabled=1).rvo_enabled == 1      # a raw override is handed on as it is (and refused by cavoid_create)


def test_header_declares_the_form_and_the_field_value():
    from rl_collision_avoidance_amd import _lib
    header = open(os.path.join(ROOT, "include", "cavoid.h")).read()
    m = re.search(r"CAVOID_FORM_CROWD_RVO\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == 9 and _lib.STEP_FORMS[9] == "CROWD_RVO" and len(_lib.STEP_FORMS) == 10
    m = re.search(r"CAVOID_RVO_WAVE\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == _lib.RVO_WAVE == 2
    assert re.search(r"#define\s+CAVOID_ABI_VERSION\s+3\b", header)
    assert "gen_max_agents = 16" in header                        # what to take for ORCA at 16 agents


def test_library_exports_what_the_binding_needs():
    from rl_collision_avoidance_amd import _lib
    lib = _lib.lib()
    for name in ("cavoid_create", "cavoid_step", "cavoid_step_autoreset", "cavoid_step_autoreset_n", "cavoid_step_push", "cavoid_last_step_form"):
        assert hasattr(lib, name), name
    cfg = _lib.CavoidCfg()
    assert lib.cavoid_default_cfg(C.byref(cfg), 20, 19) == 0 and cfg.rvo_enabled == 0
    assert lib.cavoid_last_step_form(None, None) == 0


@pytest.mark.skipif(not _HAVE_LLVM, reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_crowd_rvo_kernels_are_six_and_use_no_scratch():
    text = _kernel_notes()
    step = re.findall(r"\.name:\s+(\S*crowd_rvo_kernel\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(step) == 4, step              # two buckets (32, 64) x (MODE_STEP, MODE_STEP_AUTORESET_N); reset / observe stay on crowd_kernel
    push = re.findall(r"\.name:\s+(\S*crowd_rvo_push_kernel\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(push) == 2, push
    assert all(int(size) == 0 for _, size in step + push), step + push
    assert re.findall(r"\.max_flat_workgroup_size:\s+(\d+)\s*\n\s*\.name:\s+\S*crowd_rvo_push_kernel", text) == ["128", "128"]
    assert re.findall(r"\.max_flat_workgroup_size:\s+(\d+)\s*\n\s*\.name:\s+\S*crowd_rvo_kernel", text) == ["64"] * 4
    # no static LDS: the kernels live on the crowd form's dynamic allocation, which cavoid_create's 64 KiB check covers
    static_lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\s*\n(?:(?!\s*\.name:).*\n){0,12}\s*\.name:\s+\S*crowd_rvo_", text)
    assert len(static_lds) == 6 and all(int(v) == 0 for v in static_lds), static_lds
