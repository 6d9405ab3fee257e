#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libcavoid_hip.so, instruction stream by instruction stream.

    python tools/kernel_diff.py <libA.so> <libB.so>

Every gfx950 code object of each library is disassembled (llvm-objdump -d); per symbol of its text the instruction stream is taken with
addresses and encodings stripped, which also strips the `<symbol+offset>` labels of branch targets (the branch distance itself stays
in the instruction).  The report names the symbols that are missing from B or new in B, counts the identical ones, and for every
changed one prints its instruction and MFMA counts and, from the code objects' notes, its VGPR / AGPR / scratch figures and the
occupancy its register count allows (512 unified registers per SIMD lane, granule 8, at most 8 waves).  A refactor that is meant to
leave the machine code alone is checked with this, not by eye (profiles/policy_ring_fold_resources.txt).

Needs llvm-objdump and llvm-readelf of the ROCm toolchain; no GPU.  Exit status: 0 when nothing is missing, new or changed, else 1."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("CAVOID_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
SYMBOL = re.compile(r"^[0-9a-f]+ <(.+)>:$")
NOTE_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def code_objects(lib, work):
    """paths of the gfx950 code objects of a HIP fat binary, in link order"""
    local = os.path.join(work, "lib.so")
    shutil.copy(lib, local)                                     # (--offloading extracts the bundles next to its input)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], cwd=work, check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    names = [n for n in os.listdir(work) if "amdgcn-amd-amdhsa--gfx950" in n]
    return [os.path.join(work, n) for n in sorted(names, key=lambda n: int(re.search(r"\.(\d+)\.hipv4", n).group(1)))]


def streams(obj):
    """{symbol: [instruction, ...]} of one code object: mnemonic and operands only"""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", obj], check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = SYMBOL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(" ".join(line.split("//")[0].split()))
    return out


def notes(obj):
    """{kernel symbol: {note key: int}} from the code object's metadata"""
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.DEVNULL, text=True).stdout
    out = {}
    for block in re.split(r"\n\s+- (?=\.agpr_count)", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(m.group(1)) for k in NOTE_KEYS for m in [re.search(re.escape(k) + r":\s+(\d+)", block)] if m}
    return out


def load(lib):
    """-> (number of code objects, {symbol: [(stream, notes or None), ...]} -- one entry per code object that defines the symbol)"""
    work = tempfile.mkdtemp(prefix="cavoid_kdiff_")
    try:
        objs = code_objects(lib, work)
        table = {}
        for obj in objs:
            meta = notes(obj)
            for sym, ins in streams(obj).items():
                table.setdefault(sym, []).append((ins, meta.get(sym)))
        return len(objs), table
    finally:
        shutil.rmtree(work, ignore_errors=True)


def mfma(ins):
    return sum(1 for i in ins if i.startswith(("v_mfma", "v_smfmac")))


def resources(meta):
    if meta is None:
        return "(no kernel metadata: a device function)"
    unified = meta.get(".vgpr_count", 0)                        # arch VGPRs rounded up to 4, plus the AGPRs
    waves = min(8, 512 // max(8, (unified + 7) // 8 * 8))
    return ("VGPRs+AGPRs: %d\tAGPRs: %d\tSGPRs: %d\tScratchSize [bytes/lane]: %d\tOccupancy by registers [waves/SIMD]: %d\tSGPRs Spill: %d\t"
            "VGPRs Spill: %d" % (unified, meta.get(".agpr_count", 0), meta.get(".sgpr_count", 0), meta.get(".private_segment_fixed_size", 0),
                                 waves, meta.get(".sgpr_spill_count", 0), meta.get(".vgpr_spill_count", 0)))


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    (na, a), (nb, b) = load(argv[1]), load(argv[2])
    count = lambda t: sum(len(v) for v in t.values())
    print("code objects: %d / %d; symbols: %d / %d" % (na, nb, count(a), count(b)))
    missing = sorted(s for s in a for _ in range(max(0, len(a[s]) - len(b.get(s, [])))))
    new = sorted(s for s in b for _ in range(max(0, len(b[s]) - len(a.get(s, [])))))
    print("missing: %s" % missing)
    print("new: %s" % new)
    identical, changed = 0, []
    for sym in sorted(a):
        for (ia, ma), (ib, mb) in zip(a[sym], b.get(sym, [])):
            if ia == ib:
                identical += 1
            else:
                changed.append((sym, ia, ma, ib, mb))
    print("identical: %d, changed: %d" % (identical, len(changed)))
    print("instructions (with each symbol's trailing padding): %d / %d, MFMA: %d / %d" %
          (sum(len(i) for v in a.values() for i, _ in v), sum(len(i) for v in b.values() for i, _ in v),
           sum(mfma(i) for v in a.values() for i, _ in v), sum(mfma(i) for v in b.values() for i, _ in v)))
    for sym, ia, ma, ib, mb in changed:
        differing = sum(1 for x, y in zip(ia, ib) if x != y) + abs(len(ia) - len(ib))
        print("%s\tinstructions %d -> %d\tMFMA %d -> %d\tpositions that differ: %d" % (sym, len(ia), len(ib), mfma(ia), mfma(ib), differing))
        print("  A\t" + resources(ma))
        print("  B\t" + resources(mb))
    return 1 if missing or new or changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
