"""Gathers on resident buffers (blz_ntt_vec_gather), the part that needs no device: the entry point and the three-field view
struct exist in every layer with the documented signature and field order, a null handle is refused whatever else is passed,
and the shipped gfx950 code object holds what the kernels promise - every k_gather_* kernel exists for the three scalar fields
and nothing else, the same set per field, stays out of scratch and within 128 VGPRs (the bound tests/test_ntt_horner.py holds
its siblings to), and none of them falls into a kernel family another ISA test counts."""
import ctypes
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, kernel_scratch, kernel_vgprs, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
VIEW_FIELDS = ("offset", "stride", "len")


def test_entry_point_and_view_struct_in_every_layer():
    hdr = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+blz_ntt_vec_gather\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*size_t\s+buf_dst\s*,\s*const\s+blz_vec_arg\s*\*\s*a\s*,"
                     r"\s*const\s+blz_vec_view\s*\*\s*v\s*\)\s*;", code)
    assert re.search(r"typedef\s+struct\s+blz_vec_view\s*\{\s*uint64_t\s+offset\s*;\s*uint64_t\s+stride\s*;\s*uint64_t\s+len\s*;\s*\}"
                     r"\s*blz_vec_view\s*;", code)
    # behind blz_ntt_vec_horner and ahead of the bank permutations; nothing of it above blz_ntt_vec_horner
    assert code.index("blz_ntt_vec_horner") < code.index("blz_vec_view") < code.index("blz_ntt_vec_gather")
    assert code.index("blz_ntt_vec_gather") < code.index("blz_ntt_banks_preprocess_device")
    assert hdr.index("blz_ntt_vec_horner(blz_ntt") < hdr.index("Gathers on resident buffers")
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzVecArg, BlzVecView
    assert "blz_ntt_vec_gather" in EXPORTED_SYMBOLS
    assert EXPORTED_SYMBOLS.index("blz_ntt_vec_horner") < EXPORTED_SYMBOLS.index("blz_ntt_vec_gather") < EXPORTED_SYMBOLS.index("blz_ntt_banks_preprocess_device")
    assert _SIGS["blz_ntt_vec_gather"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(BlzVecArg), ctypes.POINTER(BlzVecView)])
    assert getattr(ctypes.CDLL(LIB), "blz_ntt_vec_gather") is not None
    assert [(n, t) for n, t in BlzVecView._fields_] == [(n, ctypes.c_uint64) for n in VIEW_FIELDS]
    assert ctypes.sizeof(BlzVecView) == 24
    # a null handle is refused before anything else is looked at
    L = blaze_amd.lib()
    a, v = BlzVecArg(None, 0, 0, 0), BlzVecView(0, 1, 0)
    assert L.blz_ntt_vec_gather(None, 0, ctypes.byref(a), ctypes.byref(v)) == 4
    assert L.blz_ntt_vec_gather(None, 99, None, None) == 4
    assert L.blz_ntt_vec_gather(None, 0, ctypes.byref(BlzVecArg(None, 7, 1, 3)), ctypes.byref(BlzVecView(9, 9, 1 << 40))) == 4
    # the mirrors
    from blaze_amd.ingo_ntt import NTTClient
    for m in (NTTClient.vec_gather, NTTClient.vec_rotate, NTTClient.vec_extend):
        assert callable(m) and "_vec_keep" in m.__code__.co_names, m
    hpp = _read("include", "blaze.hpp")
    assert "blz_ntt_vec_gather(" in hpp and "blz_vec_view" in hpp
    for m in ("vec_gather", "vec_rotate", "vec_extend"):
        assert re.search(rf"void\s+{m}\s*\(", hpp), m
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_vec_gather\(h: \*mut BlzNtt, buf_dst: usize, a: \*const BlzVecArg, v: \*const BlzVecView\) -> c_int;", ffi)
    assert re.search(r"#\[repr\(C\)\]\s*(#\[derive\([^\]]*\)\]\s*)?pub struct BlzVecView\s*\{\s*pub offset: u64,\s*pub stride: u64,\s*pub len: u64,?\s*\}", ffi)
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert all(f"fn {m}" in api for m in ("vec_gather", "vec_rotate", "vec_extend")) and "blz_ntt_vec_gather(" in api
    assert re.search(r"BlzVecView\s*\{\s*offset\s*,\s*stride\s*,\s*len\s*\}", api)   # by name: the order is the struct's
    # the kernels live in their own header and reach the handle through NttFieldOps
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    assert '#include "ntt_gather.hip.hpp"' in impl and "o.vec_gather" in impl
    assert re.search(r"\(\*vec_gather\)\s*\(\s*hipStream_t\s+st\s*,\s*uint32_t\s*\*\s*dst\s*,\s*NttVecArg\s+a\s*,\s*uint64_t\s+offset\s*,"
                     r"\s*uint64_t\s+stride\s*,\s*uint64_t\s+len\s*,\s*uint64_t\s+n\s*\)", _read("blaze_amd", "csrc", "ntt_engine.hpp"))
    # one operand check for every op: the gather hands it its bound, it does not carry a copy
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.count("hipMemGetAddressRange(") == 1 and ntt.count("is not a power of two") == 1


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    return kernel_vgprs(LIB), kernel_scratch(LIB)


def test_gather_kernels_stay_out_of_scratch_and_within_128_vgprs(code):
    vgprs, scratch = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_gather_", n))
    print({n: (vgprs[n], scratch[n]) for n in names})
    per_field = [[n for n in names if re.match(rf"_ZN3blz\d+k_gather_\w+?INS_{f}E", n)] for f in FIELDS]
    # a contiguous and a general variant per field
    assert len(per_field[0]) >= 2 and len({len(p) for p in per_field}) == 1, per_field
    assert sum(len(p) for p in per_field) == len(names), names    # instantiated on the three scalar fields and nothing else
    # the same kernels for every field
    assert len({tuple(re.sub(r"INS_\d+Fr_[A-Z0-9]+E", "", n) for n in p) for p in per_field}) == 1, per_field
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= 128, (n, vgprs[n])
        # the other ISA tests select kernels by these fragments: the new ones stay out of their sets
        for family in (r"k_fold_", r"k_vec_", r"k_horner_", r"k3t?_"):
            assert not re.match(rf"_ZN3blz\d+{family}", n), (n, family)
        assert "k_ntt512_rr" not in n and "poseidon" not in n
