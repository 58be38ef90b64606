"""Disassembly helpers for the CPU tests that tie bench.py's instruction-count constants to the shipped code object:
the gfx950 code objects are carved out of libblaze_hip.so's .hip_fatbin section (one clang offload bundle per translation
unit) and disassembled with the ROCm LLVM tools."""
import os
import re
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    """The text of a file of the repository, by its path from the root."""
    return open(os.path.join(ROOT, *parts)).read()


def function_body(text, head):
    """A top-level function of a source text, from `head` (as "int name(") to its closing brace in column 0."""
    body = text[text.index(head):]
    return body[:body.index("\n}\n")]


def tools_available() -> bool:
    return all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler"))


def disassemble_library(lib_path: str, tool: str = "llvm-objdump", flag: str = "-d") -> str:
    """Concatenated `llvm-objdump -d` text (or another LLVM tool's output) of every gfx950 code object in the library."""
    out = []
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib_path, fat])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for k, s in enumerate(starts):
            piece = os.path.join(td, f"b{k}.bin")
            with open(piece, "wb") as f:
                f.write(blob[s: starts[k + 1] if k + 1 < len(starts) else len(blob)])
            co = os.path.join(td, f"b{k}.co")
            r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={piece}",
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            out.append(subprocess.run([os.path.join(LLVM, tool), flag, co], capture_output=True, text=True).stdout)
    return "\n".join(out)


def kernel_vgprs(lib_path: str) -> dict:
    """{mangled kernel name: .vgpr_count} from the metadata notes of every gfx950 code object in the library."""
    notes = disassemble_library(lib_path, "llvm-readelf", "--notes")
    # (a kernel's map is sorted by key: .name comes before .vgpr_count, and no other key of the map ends in 'name')
    return {n: int(v) for n, v in re.findall(r"^\s+\.name:\s+(\S+)\n(?:(?!\s+\.name:).*\n)*?\s+\.vgpr_count:\s+(\d+)", notes, re.M)}


def kernel_scratch(lib_path: str) -> dict:
    """{mangled kernel name: .private_segment_fixed_size}, from the same notes."""
    notes = disassemble_library(lib_path, "llvm-readelf", "--notes")
    return {n: int(v) for n, v in re.findall(
        r"^\s+\.name:\s+(\S+)\n(?:(?!\s+\.name:).*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", notes, re.M)}


def function_instructions(text: str, mangled: str):
    """[(address, opcode, branch target offset or None)] of one function of the disassembly."""
    lines = text.split("\n")
    hits = [i for i, l in enumerate(lines) if l.endswith("<" + mangled + ">:")]
    if not hits:
        raise KeyError(mangled)
    start = hits[0]
    ins = []
    for l in lines[start + 1:]:
        if re.match(r"^[0-9a-f]+ <", l):
            break
        m = re.match(r"\s+(\S+)\s+(.*?)\s*//\s*([0-9A-Fa-f]+):\s*[0-9A-Fa-f ]+(?:<[^+>]+\+0x([0-9a-fA-F]+)>)?", l)
        if m:
            ins.append((int(m.group(3), 16), m.group(1), int(m.group(4), 16) if m.group(4) else None))
    return ins


def count(ins, opcode: str) -> int:
    return sum(1 for _, o, _ in ins if o == opcode)


def loops(ins):
    """[(first offset, last offset, instructions)] for every backward branch of the function"""
    base = ins[0][0]
    out = []
    for a, o, t in ins:
        if o.startswith(("s_cbranch", "s_branch")) and t is not None and base + t < a:
            out.append((t, a - base, [x for x in ins if base + t <= x[0] <= a]))
    return out
