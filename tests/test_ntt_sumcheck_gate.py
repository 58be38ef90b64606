"""The sumcheck step for caller-defined gates (blz_ntt_sumcheck_gate), the part that needs no device: the entry point, the two
structs and the four limits exist in every layer with the layout the header's comment fixes, a null handle is refused whatever
else is passed, the kernels live in their own header behind one NttFieldOps slot, the documents speak of the op, and the
shipped gfx950 code object holds what the kernels promise - k_gate_round over {pairs, quads} x the three scalar fields and
nothing else, no scratch, VGPRs within the occupancy step DESIGN.md records - beside the 33 k_sc_ kernels that were there."""
import ctypes
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, function_body, kernel_scratch, kernel_vgprs, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
NAME = "blz_ntt_sumcheck_gate"
LIMITS = {"BLZ_GATE_MAX_TABLES": 12, "BLZ_GATE_MAX_TERMS": 8, "BLZ_GATE_MAX_FACTORS": 4, "BLZ_GATE_MAX_POINTS": 6}


def _header():
    hdr = _read("include", "blaze_hip.h")
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_entry_point_in_every_layer():
    hdr, code = _header()
    arg = r"const\s+blz_vec_arg\s*\*\s*"
    assert re.search(rf"int\s+{NAME}\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*const\s+blz_sum_gate\s*\*\s*gate\s*,\s*{arg}tables\s*,\s*{arg}r\s*,"
                     r"\s*uint32_t\s+points\s*,\s*uint64_t\s+len\s*,\s*void\s*\*\s*d_out\s*\)\s*;", code)
    for name, value in LIMITS.items():
        assert re.search(rf"#define\s+{name}\s+{value}\b", code), name
    # the last of the NTT block: behind blz_ntt_sumcheck_step in the header, the library's source and the symbol table
    assert code.index("blz_ntt_sumcheck_step(") < code.index(NAME + "(") < code.index("blz_poseidon_new(")
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzSumGate, BlzVecArg
    assert EXPORTED_SYMBOLS.index(NAME) == EXPORTED_SYMBOLS.index("blz_ntt_sumcheck_step") + 1
    assert EXPORTED_SYMBOLS[EXPORTED_SYMBOLS.index(NAME) + 1].startswith("blz_poseidon_")
    P = ctypes.POINTER(BlzVecArg)
    assert _SIGS[NAME] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(BlzSumGate), P, P, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p])
    assert getattr(ctypes.CDLL(LIB), NAME) is not None
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.index("int blz_ntt_sumcheck_step(") < ntt.index(f"int {NAME}(")


def test_null_handle_is_refused_before_anything_else_is_looked_at():
    from blaze_amd._lib import BlzSumGate, BlzVecArg
    L = blaze_amd.lib()
    good, junk = BlzSumGate(1, 1, -1, 0), BlzSumGate(99, 0, -7, 5)
    good.term[0].nfactors = 1
    v, bad = BlzVecArg(None, 0, 0, 0), BlzVecArg(8, 7, 1, 3)
    r = ctypes.byref
    for args in ((r(good), r(v), None, 2, 4, 16), (r(junk), r(bad), r(bad), 77, 1 << 60, None), (None, None, None, 0, 3, 8),
                 (r(good), None, r(v), 0xffffffff, 0, None)):
        assert L.blz_ntt_sumcheck_gate(None, *args) == 4
        assert b"null handle" in L.blz_last_error_message()


def test_layout_is_the_one_the_header_fixes():
    """The header's comment gives every offset and both sizes; the C structs, the ctypes mirrors and the Rust structs agree."""
    from blaze_amd import _lib
    hdr, code = _header()
    comment = hdr[hdr.index("Layout (fixed;"):]
    comment = re.sub(r"\s*\n \*\s*", " ", comment[:comment.index("A table index may repeat")])
    term = re.search(r"blz_gate_term, (\d+) bytes:\s+0 nfactors[^|]*\| 1 negate[^|]*\| 2 \.\. 5 factor\[4\][^|]*\| 6 \.\. 7 reserved", comment)
    gate = re.search(r"blz_sum_gate, (\d+) bytes:\s+0 ntables[^|]*\| 4 nterms[^|]*\| 8 common[^|]*\| 12 reserved[^|]*\| 16 term\[8\]", comment)
    assert term and gate, comment
    T, G = _lib.BlzGateTerm, _lib.BlzSumGate
    assert ctypes.sizeof(T) == int(term.group(1)) == 8 and ctypes.sizeof(G) == int(gate.group(1)) == 80
    assert [(n, getattr(T, n).offset, getattr(T, n).size) for n, _ in T._fields_] == [("nfactors", 0, 1), ("negate", 1, 1), ("factor", 2, 4), ("reserved", 6, 2)]
    assert [(n, getattr(G, n).offset, getattr(G, n).size) for n, _ in G._fields_] == [("ntables", 0, 4), ("nterms", 4, 4), ("common", 8, 4), ("reserved", 12, 4),
                                                                                       ("term", 16, 64)]
    assert G._fields_[2][1] is ctypes.c_int32
    assert (_lib.GATE_MAX_TABLES, _lib.GATE_MAX_TERMS, _lib.GATE_MAX_FACTORS, _lib.GATE_MAX_POINTS) == tuple(LIMITS.values())
    # the C declarations, field by field in this order
    assert re.search(r"typedef\s+struct\s+blz_gate_term\s*\{\s*uint8_t\s+nfactors;\s*uint8_t\s+negate;\s*uint8_t\s+factor\[BLZ_GATE_MAX_FACTORS\];"
                     r"\s*uint8_t\s+reserved\[2\];\s*\}\s*blz_gate_term;", code)
    assert re.search(r"typedef\s+struct\s+blz_sum_gate\s*\{\s*uint32_t\s+ntables;\s*uint32_t\s+nterms;\s*int32_t\s+common;\s*uint32_t\s+reserved;"
                     r"\s*blz_gate_term\s+term\[BLZ_GATE_MAX_TERMS\];\s*\}\s*blz_sum_gate;", code)
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct BlzGateTerm \{\s*pub nfactors: u8,\s*pub negate: u8,"
                     r"\s*pub factor: \[u8; BLZ_GATE_MAX_FACTORS\],\s*pub reserved: \[u8; 2\],\s*\}", ffi)
    assert re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct BlzSumGate \{\s*pub ntables: u32,\s*pub nterms: u32,\s*pub common: i32,"
                     r"\s*pub reserved: u32,\s*pub term: \[BlzGateTerm; BLZ_GATE_MAX_TERMS\],\s*\}", ffi)
    for name, value in LIMITS.items():
        assert re.search(rf"pub const {name}: (usize|u32) = {value};", ffi), name


def test_mirrors():
    from blaze_amd.ingo_ntt import NTTClient
    f = NTTClient.sumcheck_gate
    assert callable(f) and "_vec_keep" in f.__code__.co_names and NAME in f.__code__.co_names
    assert f.__code__.co_varnames[:8] == ("self", "tables", "terms", "common", "r", "points", "length", "out")
    assert f.__defaults__ == (None, None, None, None, None)
    hpp = _read("include", "blaze.hpp")
    assert re.search(r"void\s+sumcheck_gate\s*\(\s*const\s+blz_sum_gate\s*&", hpp) and NAME + "(" in hpp
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_sumcheck_gate\(h: \*mut BlzNtt, gate: \*const BlzSumGate, tables: \*const BlzVecArg, r: \*const BlzVecArg,"
                     r"\s*points: u32,\s*len: u64,\s*d_out: \*mut c_void\) -> c_int;", ffi)
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "pub unsafe fn sumcheck_gate(" in api and NAME + "(" in api and "BlzSumGate" in api


def test_kernels_in_their_own_header_behind_one_slot():
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    eng = _read("blaze_amd", "csrc", "ntt_engine.hpp")
    assert impl.index('#include "ntt_sumcheck.hip.hpp"') < impl.index('#include "ntt_gate.hip.hpp"')
    assert "o.sumcheck_gate = " in impl and re.search(r"\(\*sumcheck_gate\)\s*\(\s*hipStream_t\s+st\s*,", eng)
    src = _read("blaze_amd", "csrc", "ntt_gate.hip.hpp")
    kernels = re.findall(r"template\s*<([^>]*)>\s*__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", src)
    assert kernels == [("class Fr, class Source", "k_gate_round")], kernels   # the gate is not a template parameter
    # the bind alone, the block reduction, the launch plan and the finish are the existing step's, not copies: the launcher
    # chooses between the two instantiations, launches, and calls ntt_sumcheck.hip.hpp for the rest
    assert "sc_block_sums<Fr>(" in src and "fold_block_tree" not in src
    launcher = function_body(re.sub(r"//[^\n]*", "", src), "int ntt_sumcheck_gate_t(")
    assert all(launcher.count(f) == 1 for f in ("sc_plan(", "sc_bind_only<Fr>(", "sc_finish<Fr>(", "hipLaunchKernelGGL("))
    assert "k_gate_round<Fr, ScQuads>" in launcher and "k_gate_round<Fr, ScPairs<false>>" in launcher
    for elsewhere in ("k_mle_round_fin<Fr>", "ntt_vec_mle_fold_t<Fr>(", "VEC_MAX_BLOCKS", "hipGetLastError", "fold_log2"):
        assert elsewhere not in src, elsewhere
    statements = re.sub(r"//[^\n]*", "", src)
    for banned in ("atomic", "alloc", "volatile", "__shared__ int", "__threadfence"):   # no atomics, no flags, no allocation
        assert banned not in statements, banned
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    # the protocol is the existing step's, by ONE call to the function the two share (tests/test_ntt_sumcheck_step.py pins what
    # it holds): nothing about pointers, overlaps or what is in flight is checked here
    body = function_body(ntt, f"int {NAME}(")
    assert body.count("ntt_step_protocol(") == 1 and "h->ops->sumcheck_gate(" in body
    for elsewhere in ("hipPointerGetAttributes", "hipMemGetAddressRange", "call.resolve(", "words_meet(", "call.begin()", "call.enqueue("):
        assert elsewhere not in body, elsewhere
    assert body.index('"null handle"') < body.index("gate->") < body.index("ntt_step_protocol(")
    assert ntt.index("int ntt_step_protocol(") < ntt.index("int blz_ntt_sumcheck_step(")


def test_documented_where_the_other_ops_are():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md"):
        assert "sumcheck_gate" in _read(doc), doc
    design = _read("DESIGN.md")
    assert "Caller-defined gates" in design and "k_gate_round<Fr, Source>" in design and "close_k" in design


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    return kernel_vgprs(LIB), kernel_scratch(LIB)


# The next occupancy step (128, 168 or 256 VGPRs: 4, 3 or 2 waves per SIMD) above what the compiler reports (DESIGN.md section 4,
# "Caller-defined gates"): pairs 209 / 232 / 233, quads 224 / 247 / 248 on BLS12-381 / BLS12-377 / BN254 - two waves per SIMD
VGPR_CAP = 256


def test_gate_kernels_stay_out_of_scratch_and_within_their_vgprs(code):
    vgprs, scratch = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_gate_", n))
    print({n: (vgprs[n], scratch[n]) for n in names})
    want = {rf"_ZN3blz\d+k_gate_roundINS_{f}E{src}EEvPjNS_7NttGateE": (f, src) for f in FIELDS for src in (r"NS_\d+ScPairsILb0EEE", r"NS_\d+ScQuadsE")}
    assert len(names) == 6
    for pat in want:   # exactly {pairs, quads} x the three scalar fields
        assert sum(1 for n in names if re.match(pat, n)) == 1, (pat, names)
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= VGPR_CAP, (n, vgprs[n])
        # the other ISA tests select kernels by these fragments: the new ones stay out of their sets
        for family in (r"k_sc_", r"k_mle_", r"k_fold_", r"k_vec_", r"k_horner_", r"k_gather_", r"k_spmv_", r"k3t?_"):
            assert not re.match(rf"_ZN3blz\d+{family}", n), (n, family)
        assert "k_ntt512_rr" not in n and "poseidon" not in n
    assert len([n for n in vgprs if re.match(r"_ZN3blz\d+k_sc_", n)]) == 33
