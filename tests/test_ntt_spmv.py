"""Sparse matrix-vector products on resident buffers (blz_ntt_vec_spmv), the part that needs no device: the entry point and the
40-byte CSR struct exist in every layer with the documented signature and field order, a null handle is refused whatever else
is passed, the pointer check of the operands exists once, and the shipped gfx950 code object holds what the kernels promise -
every k_spmv_* kernel exists for the three scalar fields and nothing else, the same set per field, stays out of scratch and
within 128 VGPRs, falls into no kernel family another ISA test counts, the variants without coefficients hold fewer multiplies
than their twins and k_spmv_carry holds no Montgomery product."""
import ctypes
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, count, disassemble_library, function_instructions, kernel_scratch, kernel_vgprs, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
CSR_FIELDS = ("d_row_ptr", "d_col", "d_val", "rows", "nnz")


def test_entry_point_and_csr_struct_in_every_layer():
    hdr = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+blz_ntt_vec_spmv\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*size_t\s+buf_dst\s*,\s*const\s+blz_vec_arg\s*\*\s*x\s*,"
                     r"\s*const\s+blz_vec_csr\s*\*\s*m\s*\)\s*;", code)
    assert re.search(r"typedef\s+struct\s+blz_vec_csr\s*\{\s*const\s+uint32_t\s*\*\s*d_row_ptr\s*;\s*const\s+uint32_t\s*\*\s*d_col\s*;"
                     r"\s*const\s+void\s*\*\s*d_val\s*;\s*uint64_t\s+rows\s*;\s*uint64_t\s+nnz\s*;\s*\}\s*blz_vec_csr\s*;", code)
    # behind blz_ntt_vec_gather and ahead of the bank permutations
    assert code.index("blz_ntt_vec_gather") < code.index("blz_vec_csr") < code.index("blz_ntt_vec_spmv")
    assert code.index("blz_ntt_vec_spmv") < code.index("blz_ntt_banks_preprocess_device")
    assert "UNSPECIFIED" in hdr[hdr.index("blz_ntt_vec_gather(blz_ntt"):hdr.index("typedef struct blz_vec_csr")]
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzVecArg, BlzVecCsr
    assert "blz_ntt_vec_spmv" in EXPORTED_SYMBOLS
    assert EXPORTED_SYMBOLS.index("blz_ntt_vec_gather") < EXPORTED_SYMBOLS.index("blz_ntt_vec_spmv") < EXPORTED_SYMBOLS.index("blz_ntt_banks_preprocess_device")
    assert _SIGS["blz_ntt_vec_spmv"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(BlzVecArg), ctypes.POINTER(BlzVecCsr)])
    assert getattr(ctypes.CDLL(LIB), "blz_ntt_vec_spmv") is not None
    assert [n for n, _ in BlzVecCsr._fields_] == list(CSR_FIELDS)
    assert [t for _, t in BlzVecCsr._fields_] == [ctypes.c_void_p] * 3 + [ctypes.c_uint64] * 2
    assert ctypes.sizeof(BlzVecCsr) == 40
    # a null handle is refused before anything else is looked at
    L = blaze_amd.lib()
    x, m = BlzVecArg(None, 0, 0, 0), BlzVecCsr(None, None, None, 0, 0)
    assert L.blz_ntt_vec_spmv(None, 0, ctypes.byref(x), ctypes.byref(m)) == 4
    assert L.blz_ntt_vec_spmv(None, 99, None, None) == 4
    assert L.blz_ntt_vec_spmv(None, 0, ctypes.byref(BlzVecArg(None, 7, 1, 3)), ctypes.byref(BlzVecCsr(8, 2, 4, 1 << 40, 1 << 50))) == 4
    # the mirrors
    from blaze_amd.ingo_ntt import NTTClient
    for f in (NTTClient.vec_spmv, NTTClient.vec_index):
        assert callable(f) and "_vec_keep" in f.__code__.co_names, f
    assert NTTClient.vec_spmv.__code__.co_varnames[:8] == ("self", "dst", "x", "col", "row_ptr", "val", "rows", "nnz")
    assert NTTClient.vec_index.__code__.co_varnames[:5] == ("self", "dst", "x", "col", "val")
    hpp = _read("include", "blaze.hpp")
    assert "blz_ntt_vec_spmv(" in hpp and "blz_vec_csr" in hpp
    for f in ("vec_spmv", "vec_index"):
        assert re.search(rf"void\s+{f}\s*\(", hpp), f
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_vec_spmv\(h: \*mut BlzNtt, buf_dst: usize, x: \*const BlzVecArg, m: \*const BlzVecCsr\) -> c_int;", ffi)
    assert re.search(r"#\[repr\(C\)\]\s*(#\[derive\([^\]]*\)\]\s*)?pub struct BlzVecCsr\s*\{\s*pub d_row_ptr: \*const u32,\s*pub d_col: \*const u32,"
                     r"\s*pub d_val: \*const c_void,\s*pub rows: u64,\s*pub nnz: u64,?\s*\}", ffi)
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert all(f"fn {f}" in api for f in ("vec_spmv", "vec_index")) and "blz_ntt_vec_spmv(" in api
    assert re.search(r"BlzVecCsr\s*\{\s*d_row_ptr\s*,\s*d_col\s*,\s*d_val\s*,\s*rows\s*,\s*nnz\s*\}", api)   # by name: the order is the struct's
    # the kernels live in their own header and reach the handle through NttFieldOps
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    assert '#include "ntt_spmv.hip.hpp"' in impl and "o.vec_spmv" in impl
    assert re.search(r"\(\*vec_spmv\)\s*\(\s*hipStream_t\s+st\s*,\s*uint32_t\s*\*\s*dst\s*,\s*NttVecArg\s+x\s*,", _read("blaze_amd", "csrc", "ntt_engine.hpp"))
    # one pointer check for every op and every array: the three arrays go through the helper the operands use
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.count("hipMemGetAddressRange(") == 1 and ntt.count("is not a power of two") == 1
    assert ntt.count("hipPointerGetAttributes(&at") == 1
    body = ntt[ntt.index("int blz_ntt_vec_spmv("):ntt.index("int blz_ntt_stream(")]
    assert all(re.search(rf'device_range\("[^"]*",\s*"{f}"', body) for f in CSR_FIELDS[:3]), body


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    return kernel_vgprs(LIB), kernel_scratch(LIB), disassemble_library(LIB)


def test_spmv_kernels_stay_out_of_scratch_and_within_128_vgprs(code):
    vgprs, scratch, _ = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_spmv_", n))
    print({n: (vgprs[n], scratch[n]) for n in names})
    per_field = [[n for n in names if re.match(rf"_ZN3blz\d+k_spmv_\w+?INS_{f}E", n)] for f in FIELDS]
    # index and tile with and without coefficients, and the carry
    assert len(per_field[0]) == 5 and len({len(p) for p in per_field}) == 1, per_field
    assert sum(len(p) for p in per_field) == len(names), names    # instantiated on the three scalar fields and nothing else
    # the same kernels for every field
    assert len({tuple(re.sub(r"INS_\d+Fr_[A-Z0-9]+E", "", n) for n in p) for p in per_field}) == 1, per_field
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= 128, (n, vgprs[n])
        # the other ISA tests select kernels by these fragments: the new ones stay out of their sets
        for family in (r"k_fold_", r"k_vec_", r"k_horner_", r"k_gather_", r"k3t?_"):
            assert not re.match(rf"_ZN3blz\d+{family}", n), (n, family)
        assert "k_ntt512_rr" not in n and "poseidon" not in n


def test_multiplies_per_kernel(code):
    """v_mad_u64_u32 is the multiplier of field.hip.hpp: a Montgomery product of 8 limbs is 128 of them, vec_canon 8 (fewer where
    the modulus has limbs the compiler folds).  The variants without coefficients take no product; the carry only adds."""
    vgprs, _, text = code
    mads = {n: count(function_instructions(text, n), "v_mad_u64_u32") for n in vgprs if re.match(r"_ZN3blz\d+k_spmv_", n)}
    print(mads)
    assert len(mads) == 15
    for f in FIELDS:
        for kernel in ("k_spmv_index", "k_spmv_tile"):
            plain, with_val = (next(v for n, v in mads.items() if re.match(rf"_ZN3blz\d+{kernel}INS_{f}ELb{b}E", n)) for b in (0, 1))
            assert plain < with_val and plain < 128 <= with_val, (f, kernel, plain, with_val)
        carry = next(v for n, v in mads.items() if re.match(rf"_ZN3blz\d+k_spmv_carryINS_{f}E", n))
        assert carry < 128, (f, carry)
