"""Build the gfx950 shared library ``libcavoid_hip.so`` in-tree with hipcc (no torch extension,
no JIT cache: the built .so travels with the source tree)."""
from __future__ import annotations

import os
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.path.join(PKG_DIR, "libcavoid_hip.so")
SOURCES = [os.path.join(CSRC, "cavoid_capi.hip"), os.path.join(CSRC, "cavoid_multistep.hip"), os.path.join(CSRC, "cavoid_rvo.hip"),
           os.path.join(CSRC, "cavoid_relay.hip"), os.path.join(CSRC, "cavoid_quad.hip"), os.path.join(CSRC, "cavoid_rollout_capi.hip"),
           os.path.join(CSRC, "cavoid_policy_capi.hip"), os.path.join(CSRC, "cavoid_comm_capi.hip"), os.path.join(CSRC, "cavoid_actor.hip"),
           os.path.join(CSRC, "cavoid_actor_rvo.hip"), os.path.join(CSRC, "cavoid_actor_frozen.hip"), os.path.join(CSRC, "cavoid_crowd.hip"),
           os.path.join(CSRC, "cavoid_policy_ws.hip"), os.path.join(CSRC, "cavoid_policy_train_ring.hip"),
           os.path.join(CSRC, "cavoid_policy_wsring.hip"), os.path.join(CSRC, "cavoid_crowd_push.hip"), os.path.join(CSRC, "cavoid_crowd_rvo.hip"),
           os.path.join(CSRC, "cavoid_crowd_actor.hip"), os.path.join(CSRC, "cavoid_policy_step.hip"), os.path.join(CSRC, "cavoid_actor_ws.hip"),
           os.path.join(CSRC, "cavoid_actor_ws_rvo.hip"), os.path.join(CSRC, "cavoid_policy_step_ws.hip"), os.path.join(CSRC, "cavoid_eval.hip"),
           os.path.join(CSRC, "cavoid_eval_rvo.hip"), os.path.join(CSRC, "cavoid_eval_frozen.hip"), os.path.join(CSRC, "cavoid_eval_ws.hip"),
           os.path.join(CSRC, "cavoid_eval_ws_rvo.hip"), os.path.join(CSRC, "cavoid_eval_ws_frozen.hip"),
           os.path.join(CSRC, "cavoid_crowd_eval.hip"), os.path.join(CSRC, "cavoid_crowd_actor_ws.hip"),
           os.path.join(CSRC, "cavoid_crowd_eval_ws.hip"), os.path.join(CSRC, "cavoid_crowd_actor_mix.hip"),
           os.path.join(CSRC, "cavoid_crowd_eval_mix.hip")]
# every header cavoid_loop_host.hpp reaches (the host path of a step-loop launch, tile and crowd forms alike): part of each unit that
# launches a step loop or cavoid_step_push, whichever kernel it instantiates
LOOP_HOST = ["cavoid_loop_host.hpp", "cavoid_crowd_actor.hpp", "cavoid_crowd.hpp", "cavoid_crowd_rvo.hpp", "cavoid_policy_crowd.hpp", "cavoid_policy_pipe.hpp",
             "cavoid_actor.hpp", "cavoid_eval.hpp", "cavoid_kernels.hpp", "cavoid_quad.hpp", "cavoid_launch.hpp", "cavoid_policy.hpp", "cavoid_policy_split.hpp",
             "cavoid_policy_host.hpp", "cavoid_rollout.hpp", "cavoid_rollout_host.hpp", "cavoid_host.hpp"]
ACTOR_HOST = ["cavoid_actor_host.hpp"] + LOOP_HOST
EVAL_HOST = ["cavoid_eval_host.hpp"] + LOOP_HOST
HEADERS = {
    "cavoid_capi.hip": ["cavoid_kernels.hpp", "cavoid_launch.hpp", "cavoid_host.hpp", "cavoid_crowd.hpp", "cavoid_crowd_rvo.hpp"],
    "cavoid_multistep.hip": ["cavoid_kernels.hpp", "cavoid_launch.hpp", "cavoid_host.hpp"],
    "cavoid_rvo.hip": ["cavoid_kernels.hpp", "cavoid_launch.hpp", "cavoid_host.hpp"],
    "cavoid_relay.hip": ["cavoid_kernels.hpp", "cavoid_relay.hpp", "cavoid_launch.hpp", "cavoid_host.hpp"],
    "cavoid_quad.hip": ["cavoid_kernels.hpp", "cavoid_quad.hpp", "cavoid_launch.hpp", "cavoid_host.hpp"],
    "cavoid_rollout_capi.hip": ["cavoid_rollout.hpp", "cavoid_rollout_host.hpp", "cavoid_host.hpp"],
    "cavoid_policy_capi.hip": ["cavoid_policy.hpp", "cavoid_policy_split.hpp", "cavoid_policy_split8.hpp", "cavoid_policy_crowd.hpp", "cavoid_policy_host.hpp",
                               "cavoid_host.hpp"],
    "cavoid_policy_train_ring.hip": ["cavoid_policy.hpp", "cavoid_policy_train_ring.hpp", "cavoid_policy_split.hpp", "cavoid_policy_host.hpp", "cavoid_host.hpp"],
    "cavoid_actor.hip": ACTOR_HOST,
    "cavoid_actor_rvo.hip": ACTOR_HOST,
    "cavoid_actor_frozen.hip": ACTOR_HOST,
    "cavoid_comm_capi.hip": ["cavoid_host.hpp"],
    "cavoid_crowd.hip": ["cavoid_kernels.hpp", "cavoid_crowd.hpp", "cavoid_crowd_rvo.hpp", "cavoid_launch.hpp", "cavoid_host.hpp"],
    "cavoid_crowd_push.hip": ["cavoid_crowd_push.hpp"] + ACTOR_HOST,
    "cavoid_crowd_rvo.hip": ["cavoid_crowd_push.hpp"] + ACTOR_HOST,
    "cavoid_crowd_actor.hip": ACTOR_HOST,
    "cavoid_policy_wsring.hip": ["cavoid_policy.hpp", "cavoid_policy_ws.hpp", "cavoid_policy_wsring.hpp", "cavoid_policy_split.hpp", "cavoid_policy_host.hpp",
                                 "cavoid_host.hpp"],
    "cavoid_policy_ws.hip": ["cavoid_policy.hpp", "cavoid_policy_ws.hpp", "cavoid_policy_split.hpp", "cavoid_policy_host.hpp", "cavoid_host.hpp"],
    "cavoid_actor_ws.hip": ["cavoid_actor_ws.hpp", "cavoid_actor_ws_host.hpp", "cavoid_policy_ws.hpp"] + ACTOR_HOST,
    "cavoid_actor_ws_rvo.hip": ["cavoid_actor_ws.hpp", "cavoid_actor_ws_host.hpp", "cavoid_policy_ws.hpp"] + LOOP_HOST,
    "cavoid_policy_step.hip": ["cavoid_policy_step.hpp", "cavoid_policy.hpp", "cavoid_policy_split.hpp", "cavoid_policy_host.hpp", "cavoid_host.hpp"],
    "cavoid_policy_step_ws.hip": ["cavoid_policy_step_ws.hpp", "cavoid_policy_step.hpp", "cavoid_policy.hpp", "cavoid_policy_split.hpp", "cavoid_policy_host.hpp",
                                  "cavoid_host.hpp"],
    "cavoid_eval.hip": EVAL_HOST,
    "cavoid_eval_rvo.hip": EVAL_HOST,
    "cavoid_eval_frozen.hip": EVAL_HOST,
    "cavoid_eval_ws.hip": ["cavoid_eval_ws.hpp", "cavoid_eval_ws_host.hpp", "cavoid_actor_ws.hpp", "cavoid_policy_ws.hpp"] + EVAL_HOST,
    "cavoid_eval_ws_rvo.hip": ["cavoid_eval_ws.hpp", "cavoid_eval_ws_host.hpp", "cavoid_actor_ws.hpp", "cavoid_policy_ws.hpp"] + EVAL_HOST,
    "cavoid_eval_ws_frozen.hip": ["cavoid_eval_ws.hpp", "cavoid_eval_ws_host.hpp", "cavoid_actor_ws.hpp", "cavoid_policy_ws.hpp"] + EVAL_HOST,
    "cavoid_crowd_eval.hip": ["cavoid_crowd_eval.hpp"] + EVAL_HOST,
    "cavoid_crowd_actor_ws.hip": ["cavoid_crowd_actor_ws.hpp", "cavoid_actor_ws.hpp", "cavoid_policy_ws.hpp", "cavoid_policy_wsring.hpp"] + ACTOR_HOST,
    "cavoid_crowd_eval_ws.hip": ["cavoid_crowd_eval_ws.hpp", "cavoid_crowd_actor_ws.hpp", "cavoid_eval_ws.hpp", "cavoid_actor_ws.hpp", "cavoid_policy_ws.hpp",
                                 "cavoid_policy_wsring.hpp"] + EVAL_HOST,
    "cavoid_crowd_actor_mix.hip": ["cavoid_crowd_actor_mix.hpp"] + ACTOR_HOST,
    "cavoid_crowd_eval_mix.hip": ["cavoid_crowd_eval_mix.hpp", "cavoid_crowd_actor_mix.hpp", "cavoid_crowd_eval.hpp"] + EVAL_HOST,
}
# per-file extra flags.  The multi-step env kernels run their step loop inside the launch; MachineLICM would hoist every
# constant materialisation of the body (float64 polynomial coefficients, config scalars) out of that loop into
# registers live across it: 128 VGPRs + 276 B/lane of scratch instead of 128 VGPRs + 12 B (N = 4).
EXTRA_FLAGS = {"cavoid_multistep.hip": ["-mllvm", "-disable-machine-licm"], "cavoid_rvo.hip": ["-mllvm", "-disable-machine-licm"],
               "cavoid_relay.hip": ["-mllvm", "-disable-machine-licm"],
               # the fused actor kernel runs policy + env step + bookkeeping inside ONE step loop: same reason (without it the
               # GEMM loops' fragment addresses are hoisted across the loop: 256 VGPRs + 232 B/lane of scratch instead of 243 + 0)
               "cavoid_actor.hip": ["-mllvm", "-disable-machine-licm"], "cavoid_actor_rvo.hip": ["-mllvm", "-disable-machine-licm"],
               "cavoid_actor_frozen.hip": ["-mllvm", "-disable-machine-licm"],
               # the crowd form's step loop (cavoid_crowd.hpp): same reason
               "cavoid_crowd.hip": ["-mllvm", "-disable-machine-licm"],
               # crowd_push_kernel (cavoid_crowd_push.hpp) carries the same step loop
               "cavoid_crowd_push.hip": ["-mllvm", "-disable-machine-licm"],
               # crowd_rvo_kernel / crowd_rvo_push_kernel (cavoid_crowd_rvo.hpp): the same step loop with the ORCA solve inside
               "cavoid_crowd_rvo.hip": ["-mllvm", "-disable-machine-licm"],
               # crowd_actor_kernel (cavoid_crowd_actor.hpp): policy + crowd env step + bookkeeping inside one step loop, as cavoid_actor.hip
               "cavoid_crowd_actor.hip": ["-mllvm", "-disable-machine-licm"],
               # actor_ws_kernel (cavoid_actor_ws.hpp): the weight-sharing pass + env step + bookkeeping inside one step loop, as cavoid_actor.hip
               "cavoid_actor_ws.hip": ["-mllvm", "-disable-machine-licm"], "cavoid_actor_ws_rvo.hip": ["-mllvm", "-disable-machine-licm"],
               # eval_kernel (cavoid_eval.hpp): policy + env step + outcome record inside one step loop, as cavoid_actor.hip
               "cavoid_eval.hip": ["-mllvm", "-disable-machine-licm"], "cavoid_eval_rvo.hip": ["-mllvm", "-disable-machine-licm"],
               "cavoid_eval_frozen.hip": ["-mllvm", "-disable-machine-licm"],
               # eval_ws_kernel (cavoid_eval_ws.hpp): the weight-sharing pass + env step + outcome record inside one step loop, as cavoid_actor_ws.hip
               "cavoid_eval_ws.hip": ["-mllvm", "-disable-machine-licm"], "cavoid_eval_ws_rvo.hip": ["-mllvm", "-disable-machine-licm"],
               "cavoid_eval_ws_frozen.hip": ["-mllvm", "-disable-machine-licm"],
               # crowd_evaluate_kernel (cavoid_crowd_eval.hpp): the ring-form policy pass + crowd env step + outcome record inside one step loop, as
               # cavoid_crowd_actor.hip
               "cavoid_crowd_eval.hip": ["-mllvm", "-disable-machine-licm"],
               # crowd_ws_rollout_kernel (cavoid_crowd_actor_ws.hpp): the ring-form weight-sharing pass + crowd env step + bookkeeping inside one step
               # loop, as cavoid_crowd_actor.hip
               "cavoid_crowd_actor_ws.hip": ["-mllvm", "-disable-machine-licm"],
               # crowd_ws_evaluate_kernel (cavoid_crowd_eval_ws.hpp): the ring-form weight-sharing pass + crowd env step + outcome record inside one
               # step loop, as cavoid_crowd_eval.hip
               "cavoid_crowd_eval_ws.hip": ["-mllvm", "-disable-machine-licm"],
               # crowd_mix_rollout_kernel / crowd_mix_evaluate_kernel (cavoid_crowd_actor_mix.hpp, cavoid_crowd_eval_mix.hpp): crowd_actor_kernel's and
               # crowd_evaluate_kernel's step loops with the frozen network's second pass inside
               "cavoid_crowd_actor_mix.hip": ["-mllvm", "-disable-machine-licm"], "cavoid_crowd_eval_mix.hip": ["-mllvm", "-disable-machine-licm"]}
STAMP_PATH = os.path.join(PKG_DIR, "libcavoid_hip.so.stamp")
DEPS = SOURCES + [os.path.join(CSRC, h) for hs in HEADERS.values() for h in hs] + [os.path.join(ROOT, "include", "cavoid.h")]
OBJ_DIR = os.path.join(PKG_DIR, "build")
# Development variants (phase-trace build, ulp-fault builds) are test / tooling artefacts, never the product: they are linked
# NOT beside libcavoid_hip.so, so that the package directory holds exactly one library and a process that maps the product maps
# nothing else (selected with CAVOID_LIB=<path> by the tests and tools that want one, always in a child process).
# The phase-trace build goes to tests/_variants/ (the tracing tools load it from there).
VARIANT_DIR = os.path.join(ROOT, "tests", "_variants")
# The ulp-fault builds go beside the objects they are linked from, under a name that carries the digest of the sources: the library a
# test finds at variant_path() was built from THESE sources, whatever the file times say and whatever was built in the tree before
# (a variant of older sources lacks entry points the binding now requires, and an mtime can be newer than the sources it predates).
FAULT_DIR = os.path.join(OBJ_DIR, "variants")


def variant_path(name: str) -> str:
    """The ulp-fault variant `name` (e.g. "ulp2") of the current sources."""
    os.makedirs(FAULT_DIR, exist_ok=True)
    return os.path.join(FAULT_DIR, "libcavoid_hip_%s-%s.so" % (name, source_digest()[:16]))


# -ffp-contract=off: the reference env is unfused NumPy float64; keep mul/add separate so that the
# only numerical difference from the CPU oracle is the transcendental library.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


def hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP library cannot be built on this machine")


def source_digest() -> str:
    """sha256 over the flags and the contents of every source the library is built from (mtimes do not survive a
    copy of the tree to another box; contents do)."""
    import hashlib
    h = hashlib.sha256(repr((FLAGS[:5], sorted(EXTRA_FLAGS.items()))).encode())
    for d in sorted(DEPS):
        h.update(os.path.basename(d).encode())
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def is_stale() -> bool:
    """The in-tree binary does not match the in-tree sources (or is missing)."""
    if not os.path.exists(LIB_PATH) or not os.path.exists(STAMP_PATH):
        return True
    with open(STAMP_PATH) as f:
        return f.read().strip() != source_digest()


def _compile_objects(extra_flags, tag: str, force: bool, verbose: bool):
    """One object per translation unit, rebuilt only when it (or a header it includes) changed; the stale ones are
    compiled concurrently (each hipcc is single-threaded and the env kernels take ~1.5 min)."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(OBJ_DIR, exist_ok=True)
    objs, jobs = [], []
    for src in SOURCES:
        name = os.path.basename(src)
        obj = os.path.join(OBJ_DIR, name.replace(".hip", tag + ".o"))
        deps = [src, os.path.join(ROOT, "include", "cavoid.h")] + [os.path.join(CSRC, h) for h in HEADERS[name]]
        if force or not os.path.exists(obj) or any(os.path.getmtime(d) > os.path.getmtime(obj) for d in deps):
            cmd = [hipcc()] + FLAGS + EXTRA_FLAGS.get(name, []) + list(extra_flags) + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            jobs.append(cmd)
        objs.append(obj)
    if jobs:
        with ThreadPoolExecutor(max_workers=len(jobs)) as pool:
            list(pool.map(subprocess.check_call, jobs))
    return objs


def _link(objs, out: str, verbose: bool) -> str:
    # no -lrccl: cavoid_comm_capi.hip binds RCCL with dlopen at the first multi-rank call (single-GPU users and host-only
    # tests load without it; inside a PyTorch process it takes the librccl PyTorch has already mapped)
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-ldl", "-o", out]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


def build(force: bool = False, verbose: bool = False) -> str:
    if force or is_stale():
        digest = source_digest()             # of what is about to be compiled (a source edited meanwhile must read as stale)
        if os.path.exists(STAMP_PATH):
            os.remove(STAMP_PATH)
        _link(_compile_objects([], "", force, verbose), LIB_PATH, verbose)
        with open(STAMP_PATH, "w") as f:
            f.write(digest + "\n")
    return LIB_PATH


def build_trace(verbose: bool = False) -> str:
    """Development variant with in-kernel phase time stamps (tools/trace_step.py); never loaded by
    the product (select it with CAVOID_LIB=<path>)."""
    os.makedirs(VARIANT_DIR, exist_ok=True)
    out = os.path.join(VARIANT_DIR, "libcavoid_hip_trace.so")
    return _link(_compile_objects(["-DCAVOID_TRACE"], ".trace", False, verbose), out, verbose)


def build_ulp_fault(kind: int, verbose: bool = False) -> str:
    """Development variants with ONE ulp-scale arithmetic fault in the env step (-DCAVOID_DEV_ULP_FAULT=kind: 1 = a float32 product in
    the pair pass's distance, 2 = the position update contracted into fused multiply-adds, 3 = the sort key's centimetre bucket through
    float32, 4 = a float32 product in the ORCA policy's squared distance), for tests/test_gpu_tie_classifier.py: what the parity harness and its tie classifier say about faults of the size the
    classifier excuses.  Only the env kernels' translation units are recompiled (dev-only N = 4, 10); never loaded by the product."""
    import glob
    from concurrent.futures import ThreadPoolExecutor
    out = variant_path("ulp%d" % kind)
    if os.path.exists(out):                    # (its name carries the digest of the sources it was built from: these)
        return out
    build()                                    # the product's objects, current by content
    objs = _compile_objects([], "", False, verbose)
    jobs, swap = [], {}
    for name in ("cavoid_capi.hip", "cavoid_multistep.hip", "cavoid_rvo.hip", "cavoid_relay.hip"):
        src = os.path.join(CSRC, name)
        obj = os.path.join(OBJ_DIR, name.replace(".hip", ".ulp%d.o" % kind))
        # always recompiled: no variant of these sources exists, so an object of this name is of other sources, whatever its time
        jobs.append([hipcc()] + FLAGS + EXTRA_FLAGS.get(name, []) + ["-DCAVOID_DEV_ULP_FAULT=%d" % kind, "-DCAVOID_DEV_ONLY_N", "-c", src, "-o", obj])
        swap[os.path.join(OBJ_DIR, name.replace(".hip", ".o"))] = obj
    if jobs:
        if verbose:
            for j in jobs:
                print(" ".join(j), flush=True)
        with ThreadPoolExecutor(max_workers=len(jobs)) as pool:
            list(pool.map(subprocess.check_call, jobs))
    for old in glob.glob(os.path.join(FAULT_DIR, "libcavoid_hip_ulp%d-*.so" % kind)):    # variants of earlier sources
        os.remove(old)
    tmp = out + ".tmp"
    _link([swap.get(o, o) for o in objs], tmp, verbose)
    os.replace(tmp, out)                       # (the digest-named file appears only once it is complete)
    return out


def build_crowd_dev(verbose: bool = False) -> str:
    """Development variant that routes EVERY agent count >= 2 to the crowd form (-DCAVOID_DEV_CROWD_FROM_N=2, dev-only N = 4, 10 for
    the tile forms): tests/test_gpu_crowd.py holds its outputs bitwise to the product's tile forms at N = 4 and 10 -- the guard on the
    crowd kernel's copies of env_tile's statements -- and tests/test_gpu_crowd_rvo.py its wave-cooperative ORCA (rvo_enabled = 2 runs it
    at every N >= 2 here) to the tile forms' lane-serial ORCA at N = 4, 10 and 15.  Built like the ulp-fault variants; never loaded by the product."""
    import glob
    from concurrent.futures import ThreadPoolExecutor
    out = variant_path("crowd2")
    if os.path.exists(out):
        return out
    build()
    objs = _compile_objects([], "", False, verbose)
    jobs, swap = [], {}
    for name in ("cavoid_capi.hip", "cavoid_multistep.hip", "cavoid_crowd.hip", "cavoid_crowd_rvo.hip"):     # (the units that route by agent count)
        src = os.path.join(CSRC, name)
        obj = os.path.join(OBJ_DIR, name.replace(".hip", ".crowd2.o"))
        jobs.append([hipcc()] + FLAGS + EXTRA_FLAGS.get(name, []) + ["-DCAVOID_DEV_CROWD_FROM_N=2", "-DCAVOID_DEV_ONLY_N", "-c", src, "-o", obj])
        swap[os.path.join(OBJ_DIR, name.replace(".hip", ".o"))] = obj
    if verbose:
        for j in jobs:
            print(" ".join(j), flush=True)
    with ThreadPoolExecutor(max_workers=len(jobs)) as pool:
        list(pool.map(subprocess.check_call, jobs))
    for old in glob.glob(os.path.join(FAULT_DIR, "libcavoid_hip_crowd2-*.so")):
        os.remove(old)
    tmp = out + ".tmp"
    _link([swap.get(o, o) for o in objs], tmp, verbose)
    os.replace(tmp, out)
    return out


def build_plain_dist(verbose: bool = False) -> str:
    """Development variant WITHOUT the two trims of the relay step (-DCAVOID_MIRROR_DIST=0: every pair distance computed on every lane;
    -DCAVOID_RELAY_ROLE_ARGS=0: env_relay_kernel's roles read the kernel's own parameters), for tests/test_gpu_relay_trim.py, which holds
    the product bitwise to it.  Dev-only N, widened to the agent counts that test runs (3 .. 6 and 10).  Built like the ulp-fault
    variants; never loaded by the product."""
    import glob
    from concurrent.futures import ThreadPoolExecutor
    out = variant_path("plaindist")
    if os.path.exists(out):
        return out
    build()
    objs = _compile_objects([], "", False, verbose)
    jobs, swap = [], {}
    for name in ("cavoid_capi.hip", "cavoid_multistep.hip", "cavoid_rvo.hip", "cavoid_relay.hip"):      # (the units with the pair pass of the tile forms)
        src = os.path.join(CSRC, name)
        obj = os.path.join(OBJ_DIR, name.replace(".hip", ".plaindist.o"))
        jobs.append([hipcc()] + FLAGS + EXTRA_FLAGS.get(name, []) +
                    ["-DCAVOID_MIRROR_DIST=0", "-DCAVOID_RELAY_ROLE_ARGS=0", "-DCAVOID_DEV_ONLY_N", "-DCAVOID_DEV_ENV_NS=3,4,5,6,10",
                     "-DCAVOID_DEV_RELAY_NS=3,4,5,6", "-c", src, "-o", obj])
        swap[os.path.join(OBJ_DIR, name.replace(".hip", ".o"))] = obj
    if verbose:
        for j in jobs:
            print(" ".join(j), flush=True)
    with ThreadPoolExecutor(max_workers=len(jobs)) as pool:
        list(pool.map(subprocess.check_call, jobs))
    for old in glob.glob(os.path.join(FAULT_DIR, "libcavoid_hip_plaindist-*.so")):
        os.remove(old)
    tmp = out + ".tmp"
    _link([swap.get(o, o) for o in objs], tmp, verbose)
    os.replace(tmp, out)
    return out


if __name__ == "__main__":
    import sys
    if "--trace" in sys.argv:
        print(build_trace(verbose=True))
    elif "--plain-dist" in sys.argv:
        print(build_plain_dist(verbose=True))
    elif "--crowd-dev" in sys.argv:
        print(build_crowd_dev(verbose=True))
    elif "--ulp-faults" in sys.argv:
        for kind in (1, 2, 3, 4):
            print(build_ulp_fault(kind, verbose=True))
    else:
        print(build(force=True, verbose=True))
