"""Multilinear tables on resident buffers (blz_ntt_vec_mle_fold / _round / _eq), the part that needs no device: the three entry
points and BLZ_MLE_LOW exist in every layer with the documented signatures and in the header's order, a null handle is refused
whatever else is passed, the pointer checks still exist once, and the shipped gfx950 code object holds what the kernels
promise - the same set of k_mle_* kernels for the three scalar fields and nothing else, no scratch, at most 128 VGPRs, no name
another ISA test counts, a Montgomery product in the fold and in the equality table.  The round's kernels are the sumcheck
step's (test_ntt_sumcheck_step.py)."""
import ctypes
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, count, disassemble_library, function_instructions, kernel_scratch, kernel_vgprs, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
ENTRY_POINTS = ("blz_ntt_vec_mle_fold", "blz_ntt_vec_mle_round", "blz_ntt_vec_mle_eq")
ARG = r"const\s+blz_vec_arg\s*\*\s*"


def test_entry_points_in_every_layer():
    hdr = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(rf"int\s+blz_ntt_vec_mle_fold\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*uint32_t\s+flags\s*,\s*{ARG}dst\s*,\s*{ARG}a\s*,\s*{ARG}r\s*,"
                     r"\s*uint64_t\s+len\s*\)\s*;", code)
    assert re.search(rf"int\s+blz_ntt_vec_mle_round\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*uint32_t\s+flags\s*,\s*{ARG}a\s*,\s*{ARG}b\s*,\s*{ARG}c\s*,"
                     r"\s*uint32_t\s+points\s*,\s*uint64_t\s+len\s*,\s*void\s*\*\s*d_out\s*\)\s*;", code)
    assert re.search(rf"int\s+blz_ntt_vec_mle_eq\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*{ARG}dst\s*,\s*const\s+void\s*\*\s*d_point\s*,\s*uint32_t\s+m\s*\)\s*;", code)
    assert re.search(r"#define\s+BLZ_MLE_LOW\s+1u\b", code)
    # behind blz_ntt_vec_spmv and ahead of the bank permutations, fold - round - eq
    order = [code.index(s + "(") for s in ("blz_ntt_vec_spmv",) + ENTRY_POINTS + ("blz_ntt_banks_preprocess_device",)]
    assert order == sorted(order), order
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzVecArg
    order = [EXPORTED_SYMBOLS.index(s) for s in ("blz_ntt_vec_spmv",) + ENTRY_POINTS + ("blz_ntt_banks_preprocess_device",)]
    assert order == list(range(order[0], order[0] + 5)), order
    P = ctypes.POINTER(BlzVecArg)
    assert _SIGS["blz_ntt_vec_mle_fold"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, P, P, P, ctypes.c_uint64])
    assert _SIGS["blz_ntt_vec_mle_round"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, P, P, P, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p])
    assert _SIGS["blz_ntt_vec_mle_eq"] == (ctypes.c_int, [ctypes.c_void_p, P, ctypes.c_void_p, ctypes.c_uint32])
    # the ops on the buffers: what the header declares is what _SIGS holds, in the header's order
    declared = re.findall(r"\bint\s+(blz_ntt_vec_\w+)\s*\(", code)
    assert declared == [s for s in EXPORTED_SYMBOLS if s.startswith("blz_ntt_vec_")], declared
    cdll = ctypes.CDLL(LIB)
    for s in ENTRY_POINTS:
        assert getattr(cdll, s) is not None
    # a null handle is refused before anything else is looked at
    L = blaze_amd.lib()
    v, junk = BlzVecArg(None, 0, 0, 0), BlzVecArg(8, 7, 1, 3)
    assert L.blz_ntt_vec_mle_fold(None, 0, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v), 2) == 4
    assert L.blz_ntt_vec_mle_fold(None, 0xffffffff, None, None, None, 0) == 4
    assert L.blz_ntt_vec_mle_fold(None, 1, ctypes.byref(junk), ctypes.byref(junk), ctypes.byref(junk), 1 << 60) == 4
    assert L.blz_ntt_vec_mle_round(None, 0, ctypes.byref(v), None, None, 2, 2, 16) == 4
    assert L.blz_ntt_vec_mle_round(None, 2, None, None, ctypes.byref(junk), 99, 3, None) == 4
    assert L.blz_ntt_vec_mle_eq(None, ctypes.byref(v), 16, 1) == 4
    assert L.blz_ntt_vec_mle_eq(None, None, None, 99) == 4
    assert b"null handle" in L.blz_last_error_message()
    # the mirrors
    from blaze_amd.ingo_ntt import NTTClient
    assert NTTClient.MLE_LOW == 1
    for f in (NTTClient.vec_mle_fold, NTTClient.vec_mle_round, NTTClient.vec_mle_eq):
        assert callable(f) and "_vec_keep" in f.__code__.co_names, f
    assert NTTClient.vec_mle_fold.__code__.co_varnames[:6] == ("self", "dst", "a", "r", "length", "low")
    assert NTTClient.vec_mle_fold.__defaults__ == (None, False)
    assert NTTClient.vec_mle_round.__code__.co_varnames[:8] == ("self", "a", "b", "c", "points", "length", "low", "out")
    assert NTTClient.vec_mle_round.__defaults__ == (None, None, None, None, False, None)
    assert NTTClient.vec_mle_eq.__code__.co_varnames[:4] == ("self", "dst", "point", "m")
    assert NTTClient.vec_mle_eq.__defaults__ == (None,)
    hpp = _read("include", "blaze.hpp")
    for f in ("vec_mle_fold", "vec_mle_round", "vec_mle_eq"):
        assert re.search(rf"void\s+{f}\s*\(", hpp) and f"blz_ntt_{f}(" in hpp, f
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_vec_mle_fold\(h: \*mut BlzNtt, flags: u32, dst: \*const BlzVecArg, a: \*const BlzVecArg, r: \*const BlzVecArg,"
                     r"\s*len: u64\) -> c_int;", ffi)
    assert re.search(r"pub fn blz_ntt_vec_mle_round\(h: \*mut BlzNtt, flags: u32, a: \*const BlzVecArg, b: \*const BlzVecArg, c: \*const BlzVecArg,"
                     r"\s*points: u32,\s*len: u64,\s*d_out: \*mut c_void\) -> c_int;", ffi)
    assert re.search(r"pub fn blz_ntt_vec_mle_eq\(h: \*mut BlzNtt, dst: \*const BlzVecArg, d_point: \*const c_void, m: u32\) -> c_int;", ffi)
    assert re.search(r"pub const BLZ_MLE_LOW: u32 = 1;", ffi)
    order = [ffi.index(f"pub fn {s}(") for s in ("blz_ntt_vec_spmv",) + ENTRY_POINTS]
    assert order == sorted(order)
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    for f in ("vec_mle_fold", "vec_mle_round", "vec_mle_eq"):
        assert f"pub unsafe fn {f}(" in api and f"blz_ntt_{f}(" in api, f
    assert "BLZ_MLE_LOW" in api
    # the kernels live in their own header and reach the handle through NttFieldOps
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    eng = _read("blaze_amd", "csrc", "ntt_engine.hpp")
    assert '#include "ntt_mle.hip.hpp"' in impl
    for f in ("vec_mle_fold", "vec_mle_eq"):
        assert f"o.{f} = " in impl and re.search(rf"\(\*{f}\)\s*\(\s*hipStream_t\s+st\s*,", eng), f
    # one pointer check for every op: the new destinations, outputs and the point go through operand / device_range
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.count("hipMemGetAddressRange(") == 1 and ntt.count("is not a power of two") == 1
    assert ntt.count("hipPointerGetAttributes(&at") == 1
    body = ntt[ntt.index("int blz_ntt_vec_mle_fold("):ntt.index("int blz_ntt_stream(")]
    assert body.count("call.destination(") == 2 and body.count("call.resolve(") == 2
    assert re.search(r'device_range\("[^"]*",\s*"d_point"', body)
    # the round is the sumcheck step's PRODUCT gate without r: its entry point goes through that entry of NttFieldOps
    body = body[body.index("int blz_ntt_vec_mle_round("):body.index("int blz_ntt_vec_mle_eq(")]
    assert "h->ops->sumcheck_step(" in body and "o.vec_mle_round" not in impl and "(*vec_mle_round)" not in eng
    # documented where the other ops are
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md"):
        text = _read(doc)
        assert all(f in text for f in ("vec_mle_fold", "vec_mle_round", "vec_mle_eq")), doc


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    return kernel_vgprs(LIB), kernel_scratch(LIB), disassemble_library(LIB)


def _kernel(names, pattern):
    hit = [n for n in names if re.match(rf"_ZN3blz\d+{pattern}", n)]
    assert len(hit) == 1, (pattern, hit)
    return hit[0]


def test_mle_kernels_stay_out_of_scratch_and_within_their_vgprs(code):
    vgprs, scratch, _ = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_mle_", n))
    print({n: (vgprs[n], scratch[n]) for n in names})
    per_field = [[n for n in names if re.match(rf"_ZN3blz\d+k_mle_\w+?INS_{f}E", n)] for f in FIELDS]
    # fold x 2 pairings, round_fin, eq
    assert len(per_field[0]) == 4 and len({len(p) for p in per_field}) == 1, per_field
    assert sum(len(p) for p in per_field) == len(names), names    # instantiated on the three scalar fields and nothing else
    assert len({tuple(re.sub(r"INS_\d+Fr_[A-Z0-9]+E", "", n) for n in p) for p in per_field}) == 1, per_field
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= 128, (n, vgprs[n])
        # the other ISA tests select kernels by these fragments: the new ones stay out of their sets
        for family in (r"k_sc_", r"k_fold_", r"k_vec_", r"k_horner_", r"k_gather_", r"k_spmv_", r"k3t?_"):
            assert not re.match(rf"_ZN3blz\d+{family}", n), (n, family)
        assert "k_ntt512_rr" not in n and "poseidon" not in n


def test_multiplies_per_kernel(code):
    """v_mad_u64_u32 is the multiplier of field.hip.hpp: a Montgomery product of 8 limbs is 128 of them, vec_canon at most 8.
    The fold holds the product of its loop (and r's conversion), the equality table its doubling's and its outer word's."""
    vgprs, _, text = code
    mads = {n: count(function_instructions(text, n), "v_mad_u64_u32") for n in vgprs if re.match(r"_ZN3blz\d+k_mle_", n)}
    print(mads)
    assert len(mads) == 12
    for f in FIELDS:
        for low in (0, 1):
            assert mads[_kernel(mads, rf"k_mle_foldINS_{f}ELb{low}E")] >= 128, (f, low)
        assert mads[_kernel(mads, rf"k_mle_eqINS_{f}E")] >= 128, f
