"""Folds along a resident buffer (blz_ntt_vec_reduce, blz_ntt_vec_scan), the part that needs no device: the two entry points
exist in every layer, and the shipped gfx950 code object holds what the kernels promise - every k_fold_* kernel of the three
scalar fields stays out of scratch and within 128 VGPRs (four waves per SIMD, the element-wise kernels' bound), and the
streaming loops of the inner product and of the evaluation hold the multiply-adds of ONE field product per element, not two.
One product's figure is read from the same code object: the loop of k_ntt_ninv<Fr> is one fp_mul and nothing else.

(The MSM tail's k_fold_hot / k_fold_hot_row share the stem; they are kernels over the base fields Fq and none of this test's
business: the kernels meant here are the k_fold_* instantiated on a scalar field Fr.)"""
import ctypes
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, count, disassemble_library, function_instructions, kernel_scratch, kernel_vgprs, loops, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
PART = "_ZN3blz11k_fold_partINS_{f}ELi{op}EEEvPjNS_9NttVecArgES3_mi"
NINV = "_ZN3blz10k_ntt_ninvINS_{f}EEEvPji"
# per field: the three reductions' two kernels each, and the scan's up / down kernels for {SUM, PROD} x {wire words, totals}
STEMS = {"k_fold_part": 3, "k_fold_fin": 3, "k_fold_scan_up": 4, "k_fold_scan_down": 4}


def test_entry_points_in_every_layer():
    hdr = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+blz_ntt_vec_reduce\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*int\s+op\s*,\s*const\s+blz_vec_arg\s*\*\s*a\s*,"
                     r"\s*const\s+blz_vec_arg\s*\*\s*b\s*,\s*void\s*\*\s*d_out\s*\)\s*;", code)
    assert re.search(r"int\s+blz_ntt_vec_scan\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*int\s+op\s*,\s*uint32_t\s+flags\s*,\s*size_t\s+buf_dst\s*,"
                     r"\s*const\s+blz_vec_arg\s*\*\s*a\s*,\s*void\s*\*\s*d_total\s*\)\s*;", code)
    for k, name in enumerate(("SUM", "DOT", "EVAL")):
        assert re.search(rf"BLZ_FOLD_{name}\s*=\s*{k}\b", code), name
    for k, name in enumerate(("SUM", "PROD")):
        assert re.search(rf"BLZ_SCAN_{name}\s*=\s*{k}\b", code), name
    assert re.search(r"#define\s+BLZ_SCAN_EXCLUSIVE\s+1u\b", code)
    # behind blz_ntt_vec_op, whose enum stays as it is; and the header says that the folds see positions
    assert code.index("blz_ntt_vec_op") < code.index("enum blz_fold_op") < code.index("blz_ntt_vec_reduce") < code.index("blz_ntt_vec_scan")
    assert not re.search(r"BLZ_VEC_\w+\s*=\s*6\b", code)
    block = hdr[hdr.index("Reductions and prefix scans"): hdr.index("enum blz_fold_op")]
    assert "POSITIONS" in block and "0^0 = 1" in block and "z^p" in block
    from blaze_amd._lib import EXPORTED_SYMBOLS, BlzVecArg
    dll = ctypes.CDLL(LIB)
    for sym in ("blz_ntt_vec_reduce", "blz_ntt_vec_scan"):
        assert sym in EXPORTED_SYMBOLS
        assert getattr(dll, sym) is not None
    # a null handle is refused before anything else is looked at
    L = blaze_amd.lib()
    a = BlzVecArg(None, 0, 0, 0)
    assert L.blz_ntt_vec_reduce(None, 1, ctypes.byref(a), ctypes.byref(a), None) == 4
    assert L.blz_ntt_vec_reduce(None, 99, None, None, None) == 4
    assert L.blz_ntt_vec_scan(None, 1, 0, 0, ctypes.byref(a), None) == 4
    assert L.blz_ntt_vec_scan(None, 99, 99, 99, None, None) == 4
    # the mirrors
    from blaze_amd import ingo_ntt
    from blaze_amd.ingo_ntt import NTTClient
    assert callable(NTTClient.vec_reduce) and callable(NTTClient.vec_scan)
    assert [NTTClient.FOLD_SUM, NTTClient.FOLD_DOT, NTTClient.FOLD_EVAL] == [0, 1, 2]
    assert [NTTClient.SCAN_SUM, NTTClient.SCAN_PROD] == [0, 1] and NTTClient.SCAN_EXCLUSIVE == 1
    assert "_vec_keep" in ingo_ntt.NTTClient.vec_reduce.__code__.co_names and "_vec_keep" in ingo_ntt.NTTClient.vec_scan.__code__.co_names
    hpp = _read("include", "blaze.hpp")
    assert "blz_ntt_vec_reduce(" in hpp and re.search(r"void\s+vec_reduce\s*\(", hpp)
    assert "blz_ntt_vec_scan(" in hpp and re.search(r"void\s+vec_scan\s*\(", hpp)
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert "pub fn blz_ntt_vec_reduce" in ffi and "pub fn blz_ntt_vec_scan" in ffi
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "fn vec_reduce" in api and "blz_ntt_vec_reduce(" in api
    assert "fn vec_scan" in api and "blz_ntt_vec_scan(" in api
    # the kernels live in their own header, beside the element-wise ops', and reach the handle through NttFieldOps
    assert '#include "ntt_fold.hip.hpp"' in _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    eng = _read("blaze_amd", "csrc", "ntt_engine.hpp")
    assert re.search(r"\(\*vec_reduce\)\s*\(", eng) and re.search(r"\(\*vec_scan\)\s*\(", eng)


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    text = disassemble_library(LIB)
    return text, kernel_vgprs(LIB), kernel_scratch(LIB)


def test_fold_kernels_stay_out_of_scratch_and_within_128_vgprs(code):
    _, vgprs, scratch = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_fold_\w+?INS_\d+Fr_", n))
    print({n: (vgprs[n], scratch[n]) for n in names})
    assert len(names) == 3 * sum(STEMS.values()), names
    for f in FIELDS:
        for stem, want in STEMS.items():
            got = [n for n in names if re.match(rf"_ZN3blz\d+{stem}INS_{f}E", n)]
            assert len(got) == want, (stem, f, got)
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= 128, (n, vgprs[n])
        # the other ISA tests select kernels by these fragments: the new ones stay out of their sets
        assert not re.match(r"_ZN3blz\d+k_vec_", n) and not re.match(r"_ZN3blz\d+k3t?_", n)
        assert "k_ntt512_rr" not in n and "poseidon" not in n
    # ... and the element-wise kernels' count is what it was
    assert len([n for n in vgprs if re.match(r"_ZN3blz\d+k_vec_", n)]) == 3 * 8


@pytest.mark.parametrize("f", FIELDS)
def test_streaming_loops_hold_one_field_product_per_element(code, f):
    text, _, _ = code
    one = [count(body, "v_mad_u64_u32") for _, _, body in loops(function_instructions(text, NINV.format(f=f)))]
    assert len(one) == 1 and one[0] >= 8 * 8 * 2, one   # the loop of k_ntt_ninv: one fp_mul (>= N^2 for a b and for q m)
    one = one[0]
    for name, op, loads in (("DOT", 1, 4), ("EVAL", 2, 2)):
        ins = function_instructions(text, PART.format(f=f, op=op))
        all_loops = [(count(b, "v_mad_u64_u32"), count(b, "global_load_dwordx4")) for _, _, b in loops(ins)]
        # the main loop is the one that streams the operands: 2 x 16 bytes per 32-byte word, a and b (DOT) or a (EVAL)
        main = [(mads, ld) for mads, ld in all_loops if ld]
        print(f"{f} {name}: one product {one} multiply-adds; loops (multiply-adds, 16-byte global loads) {all_loops}")
        assert len(main) == 1 and main[0][1] == loads, all_loops
        assert one <= main[0][0] < 2 * one - 8, (main, one)
    # SUM has no product: what multiply-adds its loop holds are vec_canon's N single-limb ones
    ins = function_instructions(text, PART.format(f=f, op=0))
    body = [count(b, "v_mad_u64_u32") for _, _, b in loops(ins) if count(b, "global_load_dwordx4")]
    print(f"{f} SUM: {body}")
    assert len(body) == 1 and body[0] <= 8, body
    assert count(ins, "v_mad_u64_u32") == body[0]
