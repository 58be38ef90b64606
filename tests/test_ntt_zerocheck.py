"""The zerocheck step (blz_ntt_zerocheck_gate), the part that needs no device: the entry point exists in every layer with the
signature the header fixes and at its place - behind blz_ntt_gate_eval_lin, ahead of the Poseidon block -, a null handle is
refused whatever else is passed, the kernel lives in its own header behind one NttFieldOps slot and reuses the gate step's phases,
the entry point walks the shared step protocol with its own checks in a hook, the documents speak of the op, and the shipped
gfx950 code object holds what the kernel promises - k_zc_round over {pairs, quads} x the three scalar fields, no scratch, VGPRs
within k_gate_round's occupancy step, an inlined Montgomery product - beside the six k_gate_ and 33 k_sc_ kernels that were there."""
import ctypes
import inspect
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, count, disassemble_library, function_body, function_instructions, kernel_scratch, kernel_vgprs, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
NAME = "blz_ntt_zerocheck_gate"
# what the other ISA tests select kernels by: the new ones stay out of their sets
FAMILIES = (r"k_gate_", r"k_sc_", r"k_mle_", r"k_vec_", r"k_fold_", r"k_horner_", r"k_gather_", r"k_spmv_", r"k_scatter_", r"k3", r"k_geval", r"k_lineval")


def _uncommented(text):
    return re.sub(r"//[^\n]*", "", text)


def test_declared_in_the_header_between_gate_eval_lin_and_poseidon():
    hdr = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    arg = r"const\s+blz_vec_arg\s*\*\s*"
    assert re.search(rf"int\s+{NAME}\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*const\s+blz_sum_gate\s*\*\s*gate\s*,\s*{arg}tables\s*,\s*{arg}weight\s*,\s*{arg}r\s*,"
                     r"\s*uint32_t\s+points\s*,\s*uint64_t\s+len\s*,\s*void\s*\*\s*d_out\s*\)\s*;", code)
    between = code[code.index("int blz_ntt_gate_eval_lin("):code.index("blz_poseidon_new(")]
    assert re.findall(r"\bint\s+(blz_\w+)\s*\(", between) == ["blz_ntt_gate_eval_lin", NAME]
    # the comment says what the caller needs: the reconstruction, the cost, the refusal of a bind alone
    comment = hdr[hdr.index("The gate step of a ZEROCHECK"):hdr.index(f"int {NAME}(")]
    for said in ("s_i(X) = c_i eq(tau_{m-1-i}, X) u_i(X)", "W_i[q] + W_i[q + len / 4]", "EXACTLY len / 4 weight words", "points == 0 is refused",
                 "6 + 3 + 2 + 3 = 14", "BLZ_ERR_INVALID_PARAM", "a null gate, tables or weight", "r inside weight words [0, len / 4)"):
        assert said in comment, said


def test_exported_and_bound():
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzSumGate, BlzVecArg
    assert EXPORTED_SYMBOLS.index(NAME) == EXPORTED_SYMBOLS.index("blz_ntt_gate_eval_lin") + 1
    P = ctypes.POINTER(BlzVecArg)
    assert _SIGS[NAME] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(BlzSumGate), P, P, P, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p])
    assert getattr(ctypes.CDLL(LIB), NAME) is not None
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.index("int blz_ntt_sumcheck_gate(") < ntt.index(f"int {NAME}(")


def test_null_handle_is_refused_before_anything_else_is_looked_at():
    from blaze_amd._lib import BlzSumGate, BlzVecArg
    L = blaze_amd.lib()
    good, junk = BlzSumGate(1, 1, -1, 0), BlzSumGate(99, 0, -7, 5)
    good.term[0].nfactors = 1
    v, bad = BlzVecArg(None, 0, 0, 0), BlzVecArg(8, 7, 1, 3)
    r = ctypes.byref
    for args in ((r(good), r(v), r(v), None, 2, 4, 16), (r(junk), r(bad), r(bad), r(bad), 77, 1 << 60, None), (None, None, None, None, 0, 3, 8),
                 (r(good), None, None, r(v), 0xffffffff, 0, None)):
        assert getattr(L, NAME)(None, *args) == 4
        assert b"null handle" in L.blz_last_error_message()


def test_python_client_signature():
    from blaze_amd.ingo_ntt import NTTClient
    f = NTTClient.zerocheck_gate
    assert list(inspect.signature(f).parameters) == ["self", "tables", "terms", "weight", "common", "r", "points", "length", "out"]
    assert f.__defaults__ == (None, None, None, None, None)   # weight is required
    assert "_vec_keep" in f.__code__.co_names and NAME in f.__code__.co_names and "_sum_gate" in f.__code__.co_names
    assert "nothing is added for the weight" in f.__doc__


def test_mirrors():
    hpp = _read("include", "blaze.hpp")
    assert re.search(r"void\s+zerocheck_gate\s*\(\s*const\s+blz_sum_gate\s*&", hpp) and NAME + "(" in hpp
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_zerocheck_gate\(h: \*mut BlzNtt, gate: \*const BlzSumGate, tables: \*const BlzVecArg, weight: \*const BlzVecArg,"
                     r"\s*r: \*const BlzVecArg,\s*points: u32,\s*len: u64,\s*d_out: \*mut c_void\) -> c_int;", ffi)
    assert ffi.index("pub fn blz_ntt_gate_eval_lin(") < ffi.index("pub fn blz_ntt_zerocheck_gate(")
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "pub unsafe fn zerocheck_gate(" in api and NAME + "(" in api


def test_kernel_in_its_own_header_behind_one_slot():
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    eng = _read("blaze_amd", "csrc", "ntt_engine.hpp")
    assert impl.index('#include "ntt_gate.hip.hpp"') < impl.index('#include "ntt_zerocheck.hip.hpp"')
    assert impl.count("o.zerocheck_gate = ") == 1 and len(re.findall(r"\(\*zerocheck_gate\)\s*\(\s*hipStream_t\s+st\s*,", eng)) == 1
    src = _read("blaze_amd", "csrc", "ntt_zerocheck.hip.hpp")
    kernels = re.findall(r"template\s*<([^>]*)>\s*__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", src)
    assert kernels == [("class Fr, class Source", "k_zc_round")], kernels   # the gate is data, the weight an argument
    statements = _uncommented(src)
    assert statements.count("__global__") == 1
    for banned in ("atomic", "alloc", "volatile", "__threadfence", "__shared__ int"):
        assert banned not in statements, banned
    assert "NttGate g, NttVecArg wt" in statements
    # the phases, the plan and the reduction are the gate step's and the sumcheck step's, used and not copied
    for used in ("gate_fold_quads<Fr>(", "gate_pair<Fr, Source>(", "sc_block_sums<Fr>("):
        assert used in statements, used
    for copied in ("void gate_fold_quads(", "void gate_pair(", "ScPlan sc_plan(", "void sc_block_sums(", "int sc_finish(", "fold_block_tree", "k_mle_round_fin",
                   "VEC_MAX_BLOCKS", "hipGetLastError"):
        assert copied not in statements, copied
    launcher = function_body(statements, "int ntt_zerocheck_gate_t(")
    assert all(launcher.count(f) == 1 for f in ("sc_plan(", "sc_finish<Fr>(", "hipLaunchKernelGGL("))
    assert "k_zc_round<Fr, ScQuads>" in launcher and "k_zc_round<Fr, ScPairs<false>>" in launcher and "sc_bind_only" not in launcher
    # the weight is one more Montgomery power, in the kernel's close and in the finish alike
    assert statements.count("(int)g.close_k + 1") == 2
    # the two weight loads are issued ahead of the table folds
    kernel = statements[statements.index("void k_zc_round("):statements.index("int ntt_zerocheck_gate_t(")]
    assert kernel.index("fp_load(w2,") < kernel.index("gate_fold_quads<Fr>(") < kernel.index("fp_store(wp + i * 8, w)")
    # the gate step's header keeps its one kernel
    gate = _read("blaze_amd", "csrc", "ntt_gate.hip.hpp")
    assert re.findall(r"__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", gate) == ["k_gate_round"] and "k_zc_" not in gate


def test_entry_point_walks_the_shared_protocol():
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    body = function_body(ntt, f"int {NAME}(")
    assert body.count("ntt_step_protocol(") == 1 and body.count("ntt_zerocheck_describe(") == 1 and body.count("h->ops->zerocheck_gate(") == 1
    # the description check is blz_ntt_sumcheck_gate's own function, by reference: same limits, same messages
    assert ntt.count("ntt_zerocheck_describe = &ntt_gate_describe;") == 1 and '"gate: ' not in body
    for elsewhere in ("hipPointerGetAttributes", "hipMemGetAddressRange", "call.resolve(", "call.begin()", "call.enqueue(", "device_range("):
        assert elsewhere not in body, elsewhere
    assert body.index('"null handle"') < body.index("weight is NULL") < body.index("ntt_zerocheck_describe(") < body.index("points == 0") < body.index("ntt_step_protocol(")
    assert "blz_ntt_sumcheck_gate" in body[body.index("points == 0"):body.index("ntt_step_protocol(")]   # where a bind alone is found
    # the weight's own rules live here, in the hook, and the shared protocol keeps its three
    assert body.count("NttVecCall::words_meet(") == 2
    shared = function_body(ntt, "int ntt_step_protocol(")
    assert shared.count("NttVecCall::words_meet(") == 3 and shared.count("resolve(") == 1 and shared.count("after(") == 1
    assert shared.index("call.resolve(") < shared.index("BLZ_TRY(after(") < shared.index("call.enqueue(")
    # the existing two callers pass neither the extra operand nor the hook
    for caller in ("int blz_ntt_sumcheck_step(", "int blz_ntt_sumcheck_gate("):
        call = function_body(ntt, caller)
        assert "&w," not in call and call.count("[&](") == 1, caller


def test_documented_where_the_other_ops_are():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md"):
        assert "zerocheck_gate" in _read(doc), doc
    design = _read("DESIGN.md")
    assert "**Zerocheck step**" in design and "k_zc_round<Fr, Source>" in design
    assert "ntt_zerocheck_timing.py" in design and "ntt_zerocheck_step.json" in design
    assert "ntt_zerocheck_step.json" in _read("README.md")
    section = design[design.index("**Zerocheck step**"):]
    for kept_out in ("Out of scope", "BLZ_GATE_R1CS", "Split-eq", "BLZ_MLE_LOW", "transcript", "Linear forms"):
        assert kept_out in section, kept_out
    assert os.path.exists(os.path.join(ROOT, "tools", "ntt_zerocheck_timing.py"))


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    return kernel_vgprs(LIB), kernel_scratch(LIB), disassemble_library(LIB)


# k_gate_round's occupancy step (128, 168 or 256 VGPRs: 4, 3 or 2 waves per SIMD): the compiler reports pairs 220 / 248 / 249,
# quads 232 / 255 / 256 on BLS12-381 / BLS12-377 / BN254 ("Zerocheck step") - two waves per SIMD, as there
VGPR_CAP = 256


def test_kernels_stay_out_of_scratch_and_within_their_vgprs(code):
    vgprs, scratch, text = code
    names = sorted(n for n in vgprs if "k_zc_" in n)
    print({n: (vgprs[n], scratch[n]) for n in names})
    assert len(names) == 6, names
    for f in FIELDS:   # exactly {pairs, quads} x the three scalar fields
        for src in (r"NS_\d+ScPairsILb0EEE", r"NS_\d+ScQuadsE"):
            assert sum(1 for n in names if re.match(rf"_ZN3blz\d+k_zc_roundINS_{f}E{src}EEvPjNS_7NttGateENS_9NttVecArgE", n)) == 1, (f, src, names)
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= VGPR_CAP, (n, vgprs[n])
        assert count(function_instructions(text, n), "v_mad_u64_u32") >= 128, n   # a Montgomery product is inlined, not called
        for family in FAMILIES:
            assert not re.match(rf"_ZN3blz\d+{family}", n), (n, family)
        assert "k_ntt512_rr" not in n and "poseidon" not in n
    assert len([n for n in vgprs if re.match(r"_ZN3blz\d+k_gate_", n)]) == 6
    assert len([n for n in vgprs if re.match(r"_ZN3blz\d+k_sc_", n)]) == 33
