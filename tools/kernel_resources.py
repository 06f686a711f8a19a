"""Register, scratch and LDS use of every kernel of a built libdbsde.so, read
from the code-object metadata (no GPU), and the comparison of two builds
(profiles/put_kernel_resources.json has this format).

    python tools/kernel_resources.py THIS_LIB [PARENT_LIB OUT.json [PARENT_COMMIT]]

Each translation unit's gfx950 code object is cut out of the library's
.hip_fatbin section (uncompressed clang offload bundles) and its
amdhsa.kernels notes are read with llvm-readelf: VGPRs, AGPRs, SGPRs, scratch
(private segment, bytes per lane) and LDS (group segment, bytes per block).
Occupancy (waves per SIMD) follows from the unified register file of gfx950:
512 registers per lane, VGPRs rounded up to 8 with the AGPRs behind them,
at most 8 waves.  With two libraries: every kernel of either, the kernels
whose numbers differ, and for the fused phase kernels whether any gained
scratch or lost an occupancy step.
"""
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".private_segment_fixed_size": "scratch",
          ".group_segment_fixed_size": "lds"}
PHASE = re.compile(r"\bphase[AC]")


def fatbin(lib):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fatbin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={out}", lib,
                        os.path.join(d, "copy")], check=True)
        return open(out, "rb").read()


def code_objects(blob):
    """The gfx950 ELF of every bundle in the section."""
    pos = blob.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", blob, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                yield blob[pos + off:pos + off + size]
        pos = blob.find(MAGIC, pos + len(MAGIC))


def occupancy(vgpr, agpr):
    regs = -(-max(vgpr, 1) // 8) * 8
    regs = regs + agpr if agpr else regs
    regs = -(-regs // 8) * 8
    return max(1, min(8, 512 // regs))


def kernels(lib):
    rows = {}
    with tempfile.TemporaryDirectory() as d:
        for i, co in enumerate(code_objects(fatbin(lib))):
            path = os.path.join(d, f"co{i}.elf")
            open(path, "wb").write(co)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], capture_output=True,
                                   text=True, check=True).stdout
            cur = {}
            for line in notes.splitlines() + ["  - end"]:
                s = line.strip()
                if s.startswith("- ") and cur.get("name"):
                    rows[cur.pop("name")] = cur
                    cur = {}
                m = re.match(r"-?\s*(\.[a-z_]+):\s+(\S+)$", s)
                if not m:
                    continue
                if m.group(1) == ".name":
                    cur["name"] = m.group(2).strip("'\"")
                elif m.group(1) in FIELDS:
                    cur[FIELDS[m.group(1)]] = int(m.group(2))
    names = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for mangled, name in zip(rows, names):
        r = {k: rows[mangled].get(k, 0) for k in ("vgpr", "agpr", "sgpr", "scratch", "lds")}
        r["occupancy"] = occupancy(r["vgpr"], r["agpr"])
        out[name] = r
    return out


def main():
    this = kernels(sys.argv[1])
    if len(sys.argv) < 4:
        for n, r in sorted(this.items()):
            print(f"{n[:100]:100s} " + " ".join(f"{k} {v}" for k, v in r.items()))
        return
    parent = kernels(sys.argv[2])
    changed = {n: {"parent": parent[n], "this": this[n]} for n in sorted(this) if n in parent and parent[n] != this[n]}
    phase = sorted(n for n in this if PHASE.search(n))
    worse = [n for n in phase if n in parent and (this[n]["scratch"] > parent[n]["scratch"]
                                                  or this[n]["occupancy"] < parent[n]["occupancy"])]
    res = {"what": "code-object metadata of every kernel of libdbsde.so built from the parent commit and from this "
                   "change (hipcc -O3 --offload-arch=gfx950): VGPRs, AGPRs, SGPRs, scratch bytes per lane, LDS bytes "
                   "per block, waves per SIMD (512 unified registers per lane, 8-register granules, at most 8)",
           "parent_commit": sys.argv[4] if len(sys.argv) > 4 else None,
           "kernels": len(this), "only_in_parent": sorted(set(parent) - set(this)),
           "only_in_this": {n: this[n] for n in sorted(set(this) - set(parent))},
           "changed": changed, "fused_phase_kernels": len(phase),
           "fused_phase_kernels_with_more_scratch_or_lower_occupancy": worse,
           "this": {n: this[n] for n in sorted(this)}}
    json.dump(res, open(sys.argv[3], "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "this"}, indent=1))


if __name__ == "__main__":
    main()
