"""What the CPU tests of the library's host side share: where the built library and the toolchain are, the configuration `cavoid_create`
is handed, and the built kernels' metadata notes.  A plain module: no test file imports another."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rl_collision_avoidance_amd", "libcavoid_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("this test is about the GPU-less box")


def _create(cfg):
    from rl_collision_avoidance_amd import _lib
    h = C.c_void_p()
    return _lib.lib().cavoid_create(C.byref(cfg), 16, 0, 0, C.byref(h))


def _cfg(n, m=None):
    from rl_collision_avoidance_amd import _lib
    cfg = _lib.CavoidCfg()
    rc = _lib.lib().cavoid_default_cfg(C.byref(cfg), n, n - 1 if m is None else m)
    assert rc == 0, ("cavoid_default_cfg", n, m, rc)
    return cfg


def _kernel_notes():
    work = tempfile.mkdtemp(prefix="cavoid_notes_")
    try:
        local = os.path.join(work, "lib.so")
        shutil.copy(LIB, local)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=work, check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        text = ""
        for name in sorted(os.listdir(work)):
            if "amdgcn-amd-amdhsa--gfx950" in name:
                text += subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(work, name)], check=True,
                                       stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout
        return text
    finally:
        shutil.rmtree(work, ignore_errors=True)
