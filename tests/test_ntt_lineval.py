"""Gate evaluation with linear-form factors (blz_ntt_gate_eval_lin), the part that needs no device: the entry point exists in
every layer with the signature the header gives, the three structures have the layout the header fixes in every mirror, a null
handle is refused whatever else is passed, the kernel lives in its own header behind one NttFieldOps slot, the entry point walks
the shared protocol with a description check of its own, the documents speak of the op, and the shipped gfx950 code object holds
what the kernel promises - k_lineval over the three scalar fields and nothing else, no scratch, VGPRs within the occupancy
step DESIGN.md records, 512 bytes of LDS at the most, the products inlined."""
import ctypes
import inspect
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, count, disassemble_library, function_body, function_instructions, kernel_scratch, kernel_vgprs, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
NAME = "blz_ntt_gate_eval_lin"
FAMILIES = (r"k_gate_", r"k_vec_", r"k_sc_", r"k_mle_", r"k_fold_", r"k_horner_", r"k_gather_", r"k_spmv_", r"k_scatter_", r"k3")


def _uncommented(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_declared_in_the_header_between_gate_eval_and_poseidon():
    code = re.sub(r"/\*.*?\*/", "", _read("include", "blaze_hip.h"), flags=re.S)
    arg = r"const\s+blz_vec_arg\s*\*\s*"
    assert re.search(rf"int\s+{NAME}\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*const\s+blz_lin_gate\s*\*\s*gate\s*,\s*{arg}dst\s*,\s*{arg}tables\s*,"
                     r"\s*const\s+uint64_t\s*\*\s*rot\s*,\s*uint64_t\s+len\s*\)\s*;", code)
    assert code.index("blz_ntt_gate_eval(") < code.index(NAME + "(") < code.index("blz_poseidon_new(")
    # nothing is declared between the two evaluations
    assert not re.search(r"\bblz_[a-z0-9_]+\s*\(", code[code.index("blz_ntt_gate_eval(") + 20: code.index(NAME + "(")])
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.index("int blz_ntt_gate_eval(") < ntt.index(f"int {NAME}(")


def test_exported_and_bound():
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzLinGate, BlzVecArg
    assert NAME in EXPORTED_SYMBOLS
    assert EXPORTED_SYMBOLS.index(NAME) == EXPORTED_SYMBOLS.index("blz_ntt_gate_eval") + 1
    P = ctypes.POINTER(BlzVecArg)
    assert _SIGS[NAME] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(BlzLinGate), P, P, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64])
    assert getattr(ctypes.CDLL(LIB), NAME) is not None


def test_layout_is_the_headers_in_every_mirror():
    from blaze_amd import _lib
    from blaze_amd import ingo_ntt
    S, F, G, T = _lib.BlzLinSummand, _lib.BlzLinForm, _lib.BlzLinGate, _lib.BlzGateTerm
    assert (ctypes.sizeof(S), ctypes.sizeof(F), ctypes.sizeof(G)) == (4, 20, 240)
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [("coef", 0, 1), ("table", 1, 1), ("negate", 2, 1), ("reserved", 3, 1)]
    assert [(n, getattr(F, n).offset, getattr(F, n).size) for n, _ in F._fields_] == [("nsummands", 0, 1), ("reserved", 1, 3), ("summand", 4, 16)]
    assert [(n, getattr(G, n).offset, getattr(G, n).size) for n, _ in G._fields_] == [
        ("ntables", 0, 4), ("nterms", 4, 4), ("common", 8, 4), ("nforms", 12, 4), ("term", 16, 64), ("form", 80, 160)]
    assert dict(G._fields_)["term"]._type_ is T and dict(G._fields_)["common"] is ctypes.c_int32
    assert (_lib.LIN_MAX_TABLES, _lib.LIN_MAX_FORMS, _lib.LIN_MAX_SUMMANDS, _lib.LIN_FORM, _lib.LIN_NO_COEF) == (16, 8, 4, 0x80, 0xFF)
    assert ingo_ntt.FORM == 0x80
    code = re.sub(r"/\*.*?\*/", "", _read("include", "blaze_hip.h"), flags=re.S)
    for name, value in (("BLZ_LIN_MAX_TABLES", "16"), ("BLZ_LIN_MAX_FORMS", "8"), ("BLZ_LIN_MAX_SUMMANDS", "4"), ("BLZ_LIN_FORM", "0x80"), ("BLZ_LIN_NO_COEF", "0xFF")):
        assert re.search(rf"#define\s+{name}\s+{value}\b", code), name
    assert re.search(r"typedef\s+struct\s+blz_lin_summand\s*\{\s*uint8_t\s+coef;\s*uint8_t\s+table;\s*uint8_t\s+negate;\s*uint8_t\s+reserved;\s*\}\s*blz_lin_summand;", code)
    assert re.search(r"typedef\s+struct\s+blz_lin_form\s*\{\s*uint8_t\s+nsummands;\s*uint8_t\s+reserved\[3\];\s*blz_lin_summand\s+summand\[BLZ_LIN_MAX_SUMMANDS\];"
                     r"\s*\}\s*blz_lin_form;", code)
    assert re.search(r"typedef\s+struct\s+blz_lin_gate\s*\{\s*uint32_t\s+ntables;\s*uint32_t\s+nterms;\s*int32_t\s+common;\s*uint32_t\s+nforms;"
                     r"\s*blz_gate_term\s+term\[BLZ_GATE_MAX_TERMS\];\s*blz_lin_form\s+form\[BLZ_LIN_MAX_FORMS\];\s*\}\s*blz_lin_gate;", code)
    # blaze.hpp takes the header's structures as they are; the Rust binding spells them out
    hpp = _read("include", "blaze.hpp")
    assert re.search(r"void\s+gate_eval_lin\s*\(\s*const\s+blz_lin_gate\s*&", hpp) and "struct blz_lin_gate" not in hpp
    ffi = re.sub(r"///[^\n]*\n", "", _read("rust", "src", "driver_client", "hip_ffi.rs"))
    for name, value in (("BLZ_LIN_MAX_TABLES: usize", "16"), ("BLZ_LIN_MAX_FORMS: usize", "8"), ("BLZ_LIN_MAX_SUMMANDS: usize", "4"),
                        ("BLZ_LIN_FORM: u8", "0x80"), ("BLZ_LIN_NO_COEF: u8", "0xFF")):
        assert re.search(rf"pub const {name} = {value};", ffi), name
    assert re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct BlzLinSummand \{\s*pub coef: u8,\s*pub table: u8,\s*pub negate: u8,\s*pub reserved: u8,\s*\}", ffi)
    assert re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct BlzLinForm \{\s*pub nsummands: u8,\s*pub reserved: \[u8; 3\],"
                     r"\s*pub summand: \[BlzLinSummand; BLZ_LIN_MAX_SUMMANDS\],\s*\}", ffi)
    assert re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct BlzLinGate \{\s*pub ntables: u32,\s*pub nterms: u32,\s*pub common: i32,\s*pub nforms: u32,"
                     r"\s*pub term: \[BlzGateTerm; BLZ_GATE_MAX_TERMS\],\s*pub form: \[BlzLinForm; BLZ_LIN_MAX_FORMS\],\s*\}", ffi)


def test_null_handle_is_refused_before_anything_else_is_looked_at():
    from blaze_amd._lib import BlzLinGate, BlzVecArg
    L = blaze_amd.lib()
    good, junk = BlzLinGate(1, 1, -1, 0), BlzLinGate(99, 0, -7, 77)
    good.term[0].nfactors = 1
    junk.form[0].nsummands = 9
    v, bad = BlzVecArg(None, 0, 0, 0), BlzVecArg(8, 7, 1, 3)
    rot = (ctypes.c_uint64 * 16)(*range(16))
    r = ctypes.byref
    for args in ((r(good), r(v), r(v), None, 4), (r(junk), r(bad), r(bad), rot, 1 << 60), (None, None, None, None, 0),
                 (r(good), None, r(v), rot, 0xffffffffffffffff), (None, r(bad), None, rot, 3)):
        assert getattr(L, NAME)(None, *args) == 4
        assert b"null handle" in L.blz_last_error_message()


def test_python_client_signature():
    from blaze_amd.ingo_ntt import NTTClient
    f = NTTClient.gate_eval_lin
    assert callable(f) and "_vec_keep" in f.__code__.co_names and NAME in f.__code__.co_names
    sig = inspect.signature(f)
    assert list(sig.parameters) == ["self", "dst", "tables", "forms", "terms", "common", "rot", "length"]
    assert [sig.parameters[p].default for p in ("common", "rot", "length")] == [None, None, None]
    assert all(sig.parameters[p].default is inspect.Parameter.empty for p in ("dst", "tables", "forms", "terms"))


def test_mirrors():
    hpp = _read("include", "blaze.hpp")
    assert NAME + "(" in hpp
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_gate_eval_lin\(h: \*mut BlzNtt, gate: \*const BlzLinGate, dst: \*const BlzVecArg, tables: \*const BlzVecArg,"
                     r"\s*rot: \*const u64,\s*len: u64\) -> c_int;", ffi)
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "pub unsafe fn gate_eval_lin(" in api and NAME + "(" in api and "BlzLinGate" in api


def test_kernel_in_its_own_header_behind_one_slot():
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    eng = _read("blaze_amd", "csrc", "ntt_engine.hpp")
    assert impl.index('#include "ntt_geval.hip.hpp"') < impl.index('#include "ntt_lineval.hip.hpp"')
    assert impl.count("o.gate_eval_lin = ") == 1 and len(re.findall(r"\(\*gate_eval_lin\)\s*\(\s*hipStream_t\s+st\s*,", eng)) == 1
    src = _read("blaze_amd", "csrc", "ntt_lineval.hip.hpp")
    kernels = re.findall(r"template\s*<([^>]*)>\s*__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", src)
    assert kernels == [("class Fr", "k_lineval")], kernels   # the gate is not a template parameter, nor is the rotation
    assert src.count("__global__") == 1
    statements = _uncommented(src)
    for banned in ("atomic", "alloc", "volatile", "__threadfence"):
        assert banned not in statements, banned
    assert statements.count("__shared__") == 1 and statements.count("__syncthreads()") == 1
    assert "NttLinGate g;" in statements and "k_geval" not in statements   # the description by value; the other kernel untouched
    # every lane reaches the barrier: nothing returns out of the kernel
    kernel = statements[statements.index("void k_lineval("): statements.index("int ntt_gate_eval_lin_t(")]
    assert "return" not in kernel
    # k_geval's header keeps its one kernel
    geval = _read("blaze_amd", "csrc", "ntt_geval.hip.hpp")
    assert re.findall(r"__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", geval) == ["k_geval"] and "lineval" not in geval


def test_entry_point_walks_the_shared_protocol():
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    body = function_body(ntt, f"int {NAME}(")
    for once in ("call.destination(", "call.resolve(", "call.enqueue(", "call.begin()", "h->ops->gate_eval_lin(", "ntt_lin_gate_describe("):
        assert body.count(once) == 1, once
    for elsewhere in ("hipPointerGetAttributes", "hipMemGetAddressRange", "device_range(", "ntt_gate_describe("):
        assert elsewhere not in body, elsewhere
    assert body.index('"null handle"') < body.index("ntt_lin_gate_describe(") < body.index("call.begin()") < body.index("call.enqueue(")
    # the description check is a function of its own, called by this entry point alone, with messages of its own
    assert ntt.count("ntt_lin_gate_describe(") == 2 and ntt.count("h->ops->gate_eval_lin(") == 1
    describe = function_body(ntt, "static int ntt_lin_gate_describe(")
    assert '"gate: ' not in describe and "lin gate: " in describe
    for named in ("tables[%u]", "form[%u]", "term[%u]"):
        assert named in describe, named
    # one in-place rule for both evaluations
    assert ntt.count("ntt_gate_in_place(") == 3 and body.count("ntt_gate_in_place(") == 1
    assert ntt.count("a table written in place has rot 0") == 1


def test_documented_where_the_other_ops_are():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md"):
        assert "gate_eval_lin" in _read(doc), doc
    design = _read("DESIGN.md")
    assert "Gate evaluation with linear forms" in design and "k_lineval<Fr>" in design
    assert "ntt_lineval_timing.py" in design and "ntt_lineval_ops.json" in design
    # "Gate evaluation" no longer lists products of sums as out of scope; the new section says what still is
    assert not any("Out of scope" in l and "products of sums" in l for l in design.split("\n"))
    section = design[design.index("**Gate evaluation with linear forms**"):]
    assert "Out of scope" in section and "forms of forms" in section and "blz_ntt_sumcheck_gate" in section


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    notes = disassemble_library(LIB, "llvm-readelf", "--notes")
    lds = {n: int(v) for v, n in re.findall(r"^\s+\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\s+\.group_segment_fixed_size:).*\n)*?\s+\.name:\s+(\S+)", notes, re.M)}
    return kernel_vgprs(LIB), kernel_scratch(LIB), lds, disassemble_library(LIB)


# The next occupancy step (128, 168 or 256 VGPRs) above what the compiler reports - 93 to 104 ("Gate
# evaluation with linear forms")
VGPR_CAP = 128


def test_kernel_stays_out_of_scratch_and_within_its_vgprs(code):
    vgprs, scratch, lds, text = code
    names = sorted(n for n in vgprs if "k_lineval" in n)
    print({n: (vgprs[n], scratch[n], lds[n]) for n in names})
    assert len(names) == 3, names   # one instantiation per scalar field: every gate, rotated or not, shares it
    for f in FIELDS:
        assert sum(1 for n in names if re.match(rf"_ZN3blz\d+k_linevalINS_{f}EEEvPjNS_11LinevalArgsEm$", n)) == 1, (f, names)
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= VGPR_CAP, (n, vgprs[n])
        assert lds[n] <= 512, (n, lds[n])
        assert count(function_instructions(text, n), "v_mad_u64_u32") >= 128, n   # a Montgomery product is inlined, not called
        # the other ISA tests select kernels by these fragments: the new one stays out of their sets
        for family in FAMILIES:
            assert not re.match(rf"_ZN3blz\d+{family}", n), (n, family)
        assert "k_geval" not in n and "k_ntt512_rr" not in n and "poseidon" not in n
