"""The fused sumcheck step on resident tables (blz_ntt_sumcheck_step), the part that needs no device: the entry point and the two
gates exist in every layer with the documented signature, behind the bank permutations, a null handle is refused whatever else
is passed, the one round kernel lives in its own header and reaches the handle through NttFieldOps, the pointer checks still exist
once, and the shipped gfx950 code object holds what the kernels promise - the same set of k_sc_round instantiations (pair rounds,
vec_mle_round's included, and quad binds) for the three scalar fields and nothing else, no scratch, VGPRs within the occupancy
step DESIGN.md records, a bind that holds its fold's product, and a gate that grows with every table."""
import ctypes
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, count, disassemble_library, function_body, function_instructions, kernel_scratch, kernel_vgprs, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
NAME = "blz_ntt_sumcheck_step"
ARG = r"const\s+blz_vec_arg\s*\*\s*"


def test_entry_point_in_every_layer():
    hdr = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(rf"int\s+{NAME}\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*uint32_t\s+gate\s*,\s*{ARG}a\s*,\s*{ARG}b\s*,\s*{ARG}c\s*,\s*{ARG}d\s*,\s*{ARG}r\s*,"
                     r"\s*uint32_t\s+points\s*,\s*uint64_t\s+len\s*,\s*void\s*\*\s*d_out\s*\)\s*;", code)
    assert re.search(r"#define\s+BLZ_GATE_PRODUCT\s+0u\b", code) and re.search(r"#define\s+BLZ_GATE_R1CS\s+1u\b", code)
    assert code.index("blz_ntt_banks_postprocess_device(") < code.index(NAME + "(")
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzVecArg
    assert EXPORTED_SYMBOLS.index(NAME) == EXPORTED_SYMBOLS.index("blz_ntt_banks_postprocess_device") + 1
    P = ctypes.POINTER(BlzVecArg)
    assert _SIGS[NAME] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, P, P, P, P, P, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p])
    assert getattr(ctypes.CDLL(LIB), NAME) is not None
    # a null handle is refused before anything else is looked at
    L = blaze_amd.lib()
    v, junk = BlzVecArg(None, 0, 0, 0), BlzVecArg(8, 7, 1, 3)
    r = ctypes.byref
    assert L.blz_ntt_sumcheck_step(None, 0, r(v), None, None, None, None, 2, 4, 16) == 4
    assert b"null handle" in L.blz_last_error_message()
    assert L.blz_ntt_sumcheck_step(None, 1, r(v), r(v), r(v), r(v), r(v), 4, 8, 16) == 4
    assert L.blz_ntt_sumcheck_step(None, 99, None, None, None, r(junk), r(junk), 77, 1 << 60, None) == 4
    assert L.blz_ntt_sumcheck_step(None, 0xffffffff, r(junk), r(junk), None, r(junk), None, 0, 3, 8) == 4
    assert b"null handle" in L.blz_last_error_message()


def test_mirrors():
    from blaze_amd.ingo_ntt import NTTClient
    assert (NTTClient.GATE_PRODUCT, NTTClient.GATE_R1CS) == (0, 1)
    f = NTTClient.sumcheck_step
    assert callable(f) and "_vec_keep" in f.__code__.co_names and NAME in f.__code__.co_names
    assert f.__code__.co_varnames[:7] == ("self", "tables", "r", "gate", "points", "length", "out")
    assert f.__defaults__ == (None, NTTClient.GATE_PRODUCT, None, None, None)
    hpp = _read("include", "blaze.hpp")
    assert re.search(r"void\s+sumcheck_step\s*\(", hpp) and NAME + "(" in hpp
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_sumcheck_step\(h: \*mut BlzNtt, gate: u32, a: \*const BlzVecArg, b: \*const BlzVecArg, c: \*const BlzVecArg,"
                     r"\s*d: \*const BlzVecArg,\s*r: \*const BlzVecArg,\s*points: u32,\s*len: u64,\s*d_out: \*mut c_void\) -> c_int;", ffi)
    assert re.search(r"pub const BLZ_GATE_PRODUCT: u32 = 0;", ffi) and re.search(r"pub const BLZ_GATE_R1CS: u32 = 1;", ffi)
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "pub unsafe fn sumcheck_step(" in api and NAME + "(" in api and "BLZ_GATE_R1CS" in api and "BLZ_GATE_PRODUCT" in api


def test_kernels_in_their_own_header_behind_the_field_ops():
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    eng = _read("blaze_amd", "csrc", "ntt_engine.hpp")
    assert '#include "ntt_sumcheck.hip.hpp"' in impl
    assert "o.sumcheck_step = " in impl and re.search(r"\(\*sumcheck_step\)\s*\(\s*hipStream_t\s+st\s*,", eng)
    src = _read("blaze_amd", "csrc", "ntt_sumcheck.hip.hpp")
    # a bind alone is vec_mle_fold's launcher, not a second copy; every round polynomial - vec_mle_round's too - is ONE kernel over
    # a pair source and a gate, and the block reduction of its accumulators is written once.  The launch plan, the bind alone and
    # the finish are written once too, for this launcher and the caller-defined gate's: one launch of k_mle_round_fin, one cap
    statements = re.sub(r"//[^\n]*", "", src)
    assert statements.count("ntt_vec_mle_fold_t<Fr>(") == 1 and statements.count("k_mle_round_fin<Fr>") == 1
    assert "hipLaunchKernelGGL(k_mle_round_fin<Fr>," in function_body(statements, "int sc_finish(")
    assert statements.count("VEC_MAX_BLOCKS") == 1 and "VEC_MAX_BLOCKS" in function_body(statements, "inline ScPlan sc_plan(")
    launcher = function_body(statements, "int ntt_sumcheck_step_t(")
    assert all(launcher.count(f) == 1 for f in ("sc_plan(", "sc_bind_only<Fr>(", "sc_finish<Fr>(", "hipLaunchKernelGGL("))
    assert "hipGetLastError" not in launcher and "fold_log2" not in launcher
    both = _read("blaze_amd", "csrc", "ntt_mle.hip.hpp") + src
    kernels = re.findall(r"template\s*<([^>]*)>\s*__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", both)
    assert sorted(k for _, k in kernels) == ["k_mle_eq", "k_mle_fold", "k_mle_round_fin", "k_sc_round"], kernels
    assert [k for params, k in kernels if "GATE" in params] == ["k_sc_round"], kernels
    assert both.count("fold_block_tree<Fr>(x, acc[t]") == 1
    assert "o.vec_mle_round" not in impl and "(*vec_mle_round)" not in eng
    for banned in ("atomic", "alloc", "volatile"):   # no atomics, no flags, no allocation
        assert banned not in statements, banned
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.index("int blz_ntt_stream(") < ntt.index(f"int {NAME}(")
    assert ntt.count("hipMemGetAddressRange(") == 1 and ntt.count("is not a power of two") == 1
    assert ntt.count("hipPointerGetAttributes(&at") == 1
    # the entry point checks its gate and its tables' order, then makes ONE call to the protocol it shares with
    # blz_ntt_sumcheck_gate; the in-place and in-flight rules live there and nowhere else
    body = function_body(ntt, f"int {NAME}(")
    assert body.count("ntt_step_protocol(") == 1 and "h->ops->sumcheck_step(" in body
    for elsewhere in ("hipPointerGetAttributes", "hipMemGetAddressRange", "call.resolve(", "words_meet(", "call.begin()", "call.enqueue("):
        assert elsewhere not in body, elsewhere
    shared = function_body(ntt, "int ntt_step_protocol(")
    assert shared.count("resolve(") == 1 and "call.begin()" in shared and "call.live_length(" in shared and shared.count("call.enqueue(") == 1
    assert shared.index("call.live_length(") < shared.index("call.begin()") < shared.index("call.resolve(") < shared.index("call.enqueue(")
    assert shared.count("NttVecCall::words_meet(") == 3 and "hipPointerGetAttributes" not in shared and "hipMemGetAddressRange" not in shared
    for stem in ('"points 0 is a bind alone', "a bind and a round need len", "a periodic table cannot be folded in place", "overlap in their first len words",
                 '"r lies in the words %s%s receives"', '"d_out lies in the live words of %s%s"', "a sumcheck step takes the challenge as one device word"):
        assert ntt.count(stem) == 1 and stem in shared, stem
    assert "tab(" not in ntt and '"tables[0]"' not in ntt
    # the handle records a second written buffer beside the one the existing ops record
    assert "in_flight_buf2" in ntt and "int in_flight_buf = -1;" in ntt


def test_documented_where_the_other_ops_are():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md"):
        text = _read(doc)
        assert "sumcheck_step" in text, doc
    design = _read("DESIGN.md")
    assert "BLZ_GATE_R1CS" in design and "k_sc_round<Fr, Source, GATE, K>" in design and "ScPairs" in design and "ScQuads" in design


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    return kernel_vgprs(LIB), kernel_scratch(LIB), disassemble_library(LIB)


def _kernel(names, pattern):
    hit = [n for n in names if re.match(rf"_ZN3blz\d+{pattern}", n)]
    assert len(hit) == 1, (pattern, hit)
    return hit[0]


# The next occupancy step (128, 168 or 256 VGPRs: 4, 3 or 2 waves per SIMD) above what the compiler reports (DESIGN.md section 4,
# "Sumcheck step": pair rounds K = 1 73 - 77, K = 2 98 - 101, K = 3 118 - 128, R1CS 134 - 144; quad binds K = 1 138 - 140,
# K = 2 160 - 164, K = 3 167 - 170, R1CS 192 - 201).  k_sc_round<Fr, Source, GATE, K>: GATE 0 = PRODUCT, 1 = R1CS
FR = r"INS_\d+Fr_[A-Z0-9]+E"
PAIRS, QUADS = r"NS_\d+ScPairsILb[01]EEE", r"NS_\d+ScQuadsE"
VGPR_CAP = {rf"k_sc_round{FR}{PAIRS}Li0ELi1E": 128, rf"k_sc_round{FR}{PAIRS}Li0ELi2E": 128, rf"k_sc_round{FR}{PAIRS}Li0ELi3E": 168,
            rf"k_sc_round{FR}{PAIRS}Li1ELi4E": 168,
            rf"k_sc_round{FR}{QUADS}Li0ELi1E": 168, rf"k_sc_round{FR}{QUADS}Li0ELi2E": 168, rf"k_sc_round{FR}{QUADS}Li0ELi3E": 256,
            rf"k_sc_round{FR}{QUADS}Li1ELi4E": 256}


def test_sc_kernels_stay_out_of_scratch_and_within_their_vgprs(code):
    vgprs, scratch, _ = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_sc_", n))
    print({n: (vgprs[n], scratch[n]) for n in names})
    per_field = [[n for n in names if re.match(rf"_ZN3blz\d+k_sc_\w+?INS_{f}E", n)] for f in FIELDS]
    # six PRODUCT pair rounds (K = 1, 2, 3 x the two pairings), one R1CS pair round, four quad binds (PRODUCT K = 1, 2, 3; R1CS)
    # and nothing else - no R1CS with the low pairing, no low quads; the finish is k_mle_round_fin
    assert len(per_field[0]) == 11 and len({len(p) for p in per_field}) == 1, per_field
    assert sum(len(p) for p in per_field) == len(names), names    # instantiated on the three scalar fields and nothing else
    assert len({tuple(re.sub(r"INS_\d+Fr_[A-Z0-9]+E", "", n) for n in p) for p in per_field}) == 1, per_field
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        caps = [cap for pat, cap in VGPR_CAP.items() if re.match(rf"_ZN3blz\d+{pat}", n)]
        assert len(caps) == 1 and vgprs[n] <= caps[0], (n, vgprs[n], caps)
        # the other ISA tests select kernels by these fragments: the new ones stay out of their sets
        for family in (r"k_mle_", r"k_fold_", r"k_vec_", r"k_horner_", r"k_gather_", r"k_spmv_", r"k3t?_"):
            assert not re.match(rf"_ZN3blz\d+{family}", n), (n, family)
        assert "k_ntt512_rr" not in n and "poseidon" not in n


def test_multiplies_per_kernel(code):
    """v_mad_u64_u32 is the multiplier of field.hip.hpp: a Montgomery product of 8 limbs is 128 of them, vec_canon at most 8.  A
    pair round at K = 1 holds no product - its pairs cost two canons per operand -, every bind kernel holds the product of its
    fold (and r's conversion), and each table a gate takes adds multiply-adds."""
    vgprs, _, text = code
    mads = {n: count(function_instructions(text, n), "v_mad_u64_u32") for n in vgprs if re.match(r"_ZN3blz\d+k_sc_", n)}
    print(mads)
    assert len(mads) == 33
    for f in FIELDS:
        for low in (0, 1):
            k1, k2, k3 = (mads[_kernel(mads, rf"k_sc_roundINS_{f}ENS_\d+ScPairsILb{low}EEELi0ELi{k}E")] for k in (1, 2, 3))
            assert k1 < 128 <= k2 < k3, (f, low, k1, k2, k3)
        k1, k2, k3 = (mads[_kernel(mads, rf"k_sc_roundINS_{f}E{QUADS}Li0ELi{k}E")] for k in (1, 2, 3))
        r1cs = mads[_kernel(mads, rf"k_sc_roundINS_{f}E{QUADS}Li1ELi4E")]
        rnd = mads[_kernel(mads, rf"k_sc_roundINS_{f}ENS_\d+ScPairsILb0EEELi1ELi4E")]
        assert 128 <= k1 < k2 < k3, (f, k1, k2, k3)
        assert r1cs >= 128 and rnd >= 128, (f, r1cs, rnd)
        assert rnd < r1cs, (f, rnd, r1cs)   # the bind is the round's gate plus the folds
