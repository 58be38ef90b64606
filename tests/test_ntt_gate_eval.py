"""Gate evaluation on resident buffers (blz_ntt_gate_eval), the part that needs no device: the entry point exists in every layer
with the signature the header gives, a null handle is refused whatever else is passed, the kernel lives in its own header behind
one NttFieldOps slot, the description check is one function for both gate entry points, the documents speak of the op, and the
shipped gfx950 code object holds what the kernel promises - k_geval over the three scalar fields and nothing else, no scratch,
VGPRs within the occupancy step DESIGN.md records, the products inlined."""
import ctypes
import inspect
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, count, disassemble_library, function_body, function_instructions, kernel_scratch, kernel_vgprs, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
NAME = "blz_ntt_gate_eval"


def _uncommented(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_declared_in_the_header_ahead_of_poseidon():
    code = re.sub(r"/\*.*?\*/", "", _read("include", "blaze_hip.h"), flags=re.S)
    arg = r"const\s+blz_vec_arg\s*\*\s*"
    assert re.search(rf"int\s+{NAME}\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*const\s+blz_sum_gate\s*\*\s*gate\s*,\s*{arg}dst\s*,\s*{arg}tables\s*,"
                     r"\s*const\s+uint64_t\s*\*\s*rot\s*,\s*uint64_t\s+len\s*\)\s*;", code)
    assert code.index("blz_ntt_sumcheck_gate(") < code.index(NAME + "(") < code.index("blz_poseidon_new(")
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.index("int blz_ntt_sumcheck_gate(") < ntt.index(f"int {NAME}(")


def test_exported_and_bound():
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzSumGate, BlzVecArg
    assert NAME in EXPORTED_SYMBOLS
    P = ctypes.POINTER(BlzVecArg)
    assert _SIGS[NAME] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(BlzSumGate), P, P, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64])
    assert getattr(ctypes.CDLL(LIB), NAME) is not None


def test_null_handle_is_refused_before_anything_else_is_looked_at():
    from blaze_amd._lib import BlzSumGate, BlzVecArg
    L = blaze_amd.lib()
    good, junk = BlzSumGate(1, 1, -1, 0), BlzSumGate(99, 0, -7, 5)
    good.term[0].nfactors = 1
    v, bad = BlzVecArg(None, 0, 0, 0), BlzVecArg(8, 7, 1, 3)
    rot = (ctypes.c_uint64 * 12)(*range(12))
    r = ctypes.byref
    for args in ((r(good), r(v), r(v), None, 4), (r(junk), r(bad), r(bad), rot, 1 << 60), (None, None, None, None, 0),
                 (r(good), None, r(v), rot, 0xffffffffffffffff), (None, r(bad), None, rot, 3)):
        assert getattr(L, NAME)(None, *args) == 4
        assert b"null handle" in L.blz_last_error_message()


def test_python_client_signature():
    from blaze_amd.ingo_ntt import NTTClient
    f = NTTClient.gate_eval
    assert callable(f) and "_vec_keep" in f.__code__.co_names and NAME in f.__code__.co_names
    sig = inspect.signature(f)
    assert list(sig.parameters) == ["self", "dst", "tables", "terms", "common", "rot", "length"]
    assert [sig.parameters[p].default for p in ("common", "rot", "length")] == [None, None, None]
    assert all(sig.parameters[p].default is inspect.Parameter.empty for p in ("dst", "tables", "terms"))
    # one description builder for both gate methods
    assert "_sum_gate" in f.__code__.co_names and "_sum_gate" in NTTClient.sumcheck_gate.__code__.co_names


def test_mirrors():
    hpp = _read("include", "blaze.hpp")
    assert re.search(r"void\s+gate_eval\s*\(\s*const\s+blz_sum_gate\s*&", hpp) and NAME + "(" in hpp
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_gate_eval\(h: \*mut BlzNtt, gate: \*const BlzSumGate, dst: \*const BlzVecArg, tables: \*const BlzVecArg,"
                     r"\s*rot: \*const u64,\s*len: u64\) -> c_int;", ffi)
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "pub unsafe fn gate_eval(" in api and NAME + "(" in api


def test_kernel_in_its_own_header_behind_one_slot():
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    eng = _read("blaze_amd", "csrc", "ntt_engine.hpp")
    assert impl.index('#include "ntt_gate.hip.hpp"') < impl.index('#include "ntt_geval.hip.hpp"')
    assert "o.gate_eval = " in impl and re.search(r"\(\*gate_eval\)\s*\(\s*hipStream_t\s+st\s*,", eng)
    src = _read("blaze_amd", "csrc", "ntt_geval.hip.hpp")
    kernels = re.findall(r"template\s*<([^>]*)>\s*__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", src)
    assert kernels == [("class Fr", "k_geval")], kernels   # the gate is not a template parameter, nor is the rotation
    statements = _uncommented(src)
    for banned in ("atomic", "alloc", "volatile", "__threadfence", "__shared__"):
        assert banned not in statements, banned
    assert "NttGate g;" in statements and "k_gate_round" not in statements   # NttGate as it is, by value; the other kernel untouched
    # ntt_gate.hip.hpp and NttGate stay as they were: the sumcheck kernel takes the same description
    assert "struct NttGate {\n    uint32_t ntables, nterms;\n    int32_t common;   // < 0: none\n    uint32_t close_k;\n    uint32_t term[NTT_GATE_MAX_TERMS];\n    NttVecArg t[NTT_GATE_MAX_TABLES];\n};" in eng


def test_entry_point_walks_the_shared_protocol():
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    body = function_body(ntt, f"int {NAME}(")
    for once in ("call.destination(", "call.resolve(", "call.enqueue(", "call.begin()", "h->ops->gate_eval("):
        assert body.count(once) == 1, once
    for elsewhere in ("hipPointerGetAttributes", "hipMemGetAddressRange", "device_range("):
        assert elsewhere not in body, elsewhere
    assert ntt.count("hipPointerGetAttributes(&at") == 1 and ntt.count("hipMemGetAddressRange(") == 1
    assert body.index('"null handle"') < body.index("ntt_gate_describe(") < body.index("call.begin()") < body.index("call.enqueue(")
    # the description check is ONE function, called once by each gate entry point and by nobody else
    step = function_body(ntt, "int blz_ntt_sumcheck_gate(")
    assert step.count("ntt_gate_describe(") == 1 and body.count("ntt_gate_describe(") == 1 and ntt.count("ntt_gate_describe(") == 3
    assert ntt.count('"gate: ntables %u is not in [1, %d]"') == 1 and ntt.count("nfactors %u is not in") == 1
    for message in ("gate: ntables", "gate: nterms", "gate: common", "gate: reserved", "gate: term"):
        assert message not in body and message not in step, message


def test_documented_where_the_other_ops_are():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md"):
        assert "gate_eval" in _read(doc), doc
    design = _read("DESIGN.md")
    assert "Gate evaluation" in design and "k_geval<Fr>" in design


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    return kernel_vgprs(LIB), kernel_scratch(LIB), disassemble_library(LIB)


# The next occupancy step (128, 168 or 256 VGPRs) above what the compiler reports ("Gate evaluation")
VGPR_CAP = 128


def test_kernel_stays_out_of_scratch_and_within_its_vgprs(code):
    vgprs, scratch, text = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_geval", n))
    print({n: (vgprs[n], scratch[n]) for n in names})
    assert len(names) == 3, names   # one instantiation per scalar field: rotated and unrotated gates share it
    for f in FIELDS:
        assert sum(1 for n in names if re.match(rf"_ZN3blz\d+k_gevalINS_{f}EEEvPjNS_9GevalArgsEm$", n)) == 1, (f, names)
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= VGPR_CAP, (n, vgprs[n])
        assert count(function_instructions(text, n), "v_mad_u64_u32") >= 128, n   # a Montgomery product is inlined, not called
        # the other ISA tests select kernels by these fragments: the new one stays out of their sets
        for family in (r"k_gate_", r"k_vec_", r"k_sc_", r"k_mle_", r"k_fold_", r"k_horner_", r"k_gather_", r"k_spmv_", r"k_scatter_", r"k3"):
            assert not re.match(rf"_ZN3blz\d+{family}", n), (n, family)
        assert "k_ntt512_rr" not in n and "poseidon" not in n
