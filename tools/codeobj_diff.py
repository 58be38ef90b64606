"""Compares the gfx950 code objects of two builds of the library, kernel by kernel:

    python3 tools/codeobj_diff.py OLD/libblaze_hip.so NEW/libblaze_hip.so [--all]

Per kernel symbol: presence in either library, .vgpr_count, .sgpr_count, LDS (.group_segment_fixed_size) and private segment
size from the metadata notes, the instruction total and the mnemonic histogram's delta from the disassembly.  The out-of-line
device functions of the code objects (the group laws a kernel calls) are compared by instructions alike; they have no
resources of their own.  A symbol that moved is printed with its delta split into the instructions whose count is what a
kernel costs (multiplies, memory, LDS, DPP / SDWA, barriers, priorities: "hard") and the rest, the latter also as a share of
the symbol's total; --all prints the unchanged symbols too.

Exit code: 0 when both libraries have the same symbols with the same resources, 1 otherwise (instruction deltas are reported,
not judged).  Only the ROCm LLVM tools of tests/isa_util.py are used, and nothing but the two files is inspected."""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import isa_util  # noqa: E402

RESOURCES = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")
HARD = re.compile(r"^(v_mad_|v_mul_|global_|scratch_|ds_|buffer_|s_barrier|s_setprio)|_(dpp|sdwa)$")


def resources(lib):
    """{kernel symbol: (vgprs, sgprs, LDS bytes, private bytes)} from the metadata notes of every code object"""
    notes = isa_util.disassemble_library(lib, "llvm-readelf", "--notes")
    out = {}
    for block in re.split(r"^\s+- \.agpr_count:", notes, flags=re.M)[1:]:   # (a kernel's map is sorted by key: .agpr_count leads)
        name = re.search(r"^    \.name:\s+(\S+)", block, re.M).group(1)   # (four spaces: the kernel's own keys, not an argument's)
        out[name] = tuple(int(re.search(r"^    %s:\s+(\d+)" % re.escape(k), block, re.M).group(1)) for k in RESOURCES)
    return out


def histograms(lib):
    """{function symbol: Counter of mnemonics} over every code object (a symbol of several code objects: summed)"""
    out = collections.defaultdict(collections.Counter)
    cur = None
    for line in isa_util.disassemble_library(lib).split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out[m.group(1)]
            continue
        m = re.match(r"\s+(\S+)\s.*//\s*[0-9A-Fa-f]+:", line)
        if m and cur is not None:
            cur[m.group(1)] += 1
    return out


def delta(a, b):
    return {k: b[k] - a[k] for k in sorted(set(a) | set(b)) if a[k] != b[k]}


def main(argv):
    show_all = "--all" in argv
    libs = [a for a in argv if not a.startswith("--")]
    if len(libs) != 2 or not isa_util.tools_available():
        print(__doc__ if len(libs) != 2 else "ROCm LLVM tools not found under " + isa_util.LLVM, file=sys.stderr)
        return 2
    res = [resources(l) for l in libs]
    hist = [histograms(l) for l in libs]
    unequal = moved = 0
    for name in sorted(set(hist[0]) | set(hist[1]) | set(res[0]) | set(res[1])):
        here = [name in hist[k] or name in res[k] for k in (0, 1)]
        if not all(here):
            unequal += 1
            print(f"{name}\n    only in the {'first' if here[0] else 'second'} library")
            continue
        lines = []
        if res[0].get(name) != res[1].get(name):
            unequal += 1
            lines.append("resources " + ", ".join(f"{k} {a} -> {b}" for k, a, b in zip(RESOURCES, res[0].get(name, ()), res[1].get(name, ())) if a != b))
        d = delta(hist[0][name], hist[1][name])
        total = [sum(hist[k][name].values()) for k in (0, 1)]
        if d:
            moved += 1
            hard = {k: v for k, v in d.items() if HARD.search(k)}
            soft = sum(abs(v) for k, v in d.items() if k not in hard)
            lines.append(f"instructions {total[0]} -> {total[1]}; hard {hard or 'equal'}; rest moves {soft} = {100.0 * soft / max(total[0], 1):.3f} %: "
                         + ", ".join(f"{k} {v:+d}" for k, v in d.items() if k not in hard))
        if lines or show_all:
            r = res[1].get(name)
            print(name + ("" if r is None else "   [vgpr %d sgpr %d lds %d private %d]" % r) + (f"   {total[1]} instructions" if not d else ""))
            for l in lines:
                print("    " + l)
    print(f"{len(res[1])} kernels, {len(hist[1])} functions: {unequal} with unequal presence or resources, {moved} with moved instructions")
    return 1 if unequal else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
