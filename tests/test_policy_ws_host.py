"""CPU tests of the weight-sharing policy handle's host side (cavoid_policy_ws.hpp / cavoid_policy_ws.hip): the new C ABI is declared in
plain C and exported, cavoid_policy_create_ws tells the range it carries from the range it refuses before it looks for a device, the
Python limit mirrors the kernel's, and the built library's weight-sharing kernels use no scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests.host_support import LLVM, ROOT, _kernel_notes, _no_gpu

NEW_SYMBOLS = ("cavoid_policy_create_ws", "cavoid_policy_load_ws", "cavoid_policy_train_ws")
HEADER = os.path.join(ROOT, "include", "cavoid.h")
LIB = os.path.join(ROOT, "rl_collision_avoidance_amd", "libcavoid_hip.so")


def test_new_calls_are_declared_in_plain_c_and_exported():
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert "cavoid_policy_train_ws_buffers" in text
    assert re.search(r"#define\s+CAVOID_ABI_VERSION\s+3\b", text)
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:                                        # the header still compiles as C (no C++ crept in)
        work = tempfile.mkdtemp(prefix="cavoid_hdr_")
        try:
            src = os.path.join(work, "t.c")
            with open(src, "w") as f:
                f.write('#include "cavoid.h"\nint main(void) { cavoid_policy_train_ws_buffers b; (void)b; '
                        'return (int)sizeof(&cavoid_policy_create_ws); }\n')
            subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.dirname(HEADER), "-c", src, "-o",
                            os.path.join(work, "t.o")], check=True)
        finally:
            shutil.rmtree(work, ignore_errors=True)
    from rl_collision_avoidance_amd import _lib
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("m,code", [(1, -5), (7, -5), (19, -5), (20, -4), (64, -4), (0, -1), (65, -1)])
def test_create_ws_range_is_checked_before_the_device(m, code):
    _no_gpu()
    from rl_collision_avoidance_amd import _lib
    h = C.c_void_p()
    assert _lib.lib().cavoid_policy_create_ws(m, 11, 0, C.byref(h)) == code      # -5 ENODEVICE, -4 EUNSUPPORTED, -1 EINVAL
    assert not h.value


def test_ws_neighbour_limit_mirrors_the_kernel():
    from rl_collision_avoidance_amd.ga3c.policy_kernel import MAX_OTHERS_WS
    src = open(os.path.join(ROOT, "rl_collision_avoidance_amd", "csrc", "cavoid_policy_ws.hpp")).read()
    assert re.search(r"constexpr\s+int\s+kWsMaxOthers\s*=\s*kPolMaxOthers\s*;", src)
    assert MAX_OTHERS_WS == 19


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                    reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_ws_policy_kernels_use_no_scratch():
    text = _kernel_notes()
    found = re.findall(r"\.name:\s+(\S*policy_ws_\S*kernel\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)", text)
    names = sorted(n for n, _ in found)
    assert len(found) == 4, found            # pack, inference forward, trainer forward, trainer backward
    assert all(int(size) == 0 for _, size in found), found
    assert not any(n.endswith("crowd_kernel") or "policy_crowd_forward_kernel" in n for n in names), names
