"""Weighted (Horner) scans along a resident buffer (blz_ntt_vec_horner), the part that needs no device: the entry point exists
in every layer with the documented signature, and the shipped gfx950 code object holds what the kernels promise - every
k_horner_* kernel of the three scalar fields stays out of scratch and within 128 VGPRs (four waves per SIMD, the bound of the
k_vec_* and k_fold_* kernels), and none of them falls into a kernel family another ISA test counts."""
import ctypes
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, kernel_scratch, kernel_vgprs, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")


def test_entry_point_in_every_layer():
    hdr = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+blz_ntt_vec_horner\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*uint32_t\s+flags\s*,\s*size_t\s+buf_dst\s*,"
                     r"\s*const\s+blz_vec_arg\s*\*\s*a\s*,\s*const\s+blz_vec_arg\s*\*\s*z\s*,\s*void\s*\*\s*d_total\s*\)\s*;", code)
    assert re.search(r"#define\s+BLZ_HORNER_EXCLUSIVE\s+1u\b", code)
    assert re.search(r"#define\s+BLZ_HORNER_REVERSE\s+2u\b", code)
    # behind blz_ntt_vec_scan and ahead of the bank permutations; nothing of it above blz_ntt_vec_scan
    assert code.index("blz_ntt_vec_scan") < code.index("BLZ_HORNER_") and code.index("blz_ntt_vec_scan") < code.index("blz_ntt_vec_horner")
    assert code.index("blz_ntt_vec_horner") < code.index("blz_ntt_banks_preprocess_device")
    assert hdr.index("blz_ntt_vec_scan(") < hdr.index("Weighted (Horner) scan")
    from blaze_amd._lib import EXPORTED_SYMBOLS, BlzVecArg
    assert "blz_ntt_vec_horner" in EXPORTED_SYMBOLS
    assert getattr(ctypes.CDLL(LIB), "blz_ntt_vec_horner") is not None
    # a null handle is refused before anything else is looked at
    L = blaze_amd.lib()
    a = BlzVecArg(None, 0, 0, 0)
    assert L.blz_ntt_vec_horner(None, 0, 0, ctypes.byref(a), ctypes.byref(a), None) == 4
    assert L.blz_ntt_vec_horner(None, 99, 99, None, None, None) == 4
    # the mirrors
    from blaze_amd.ingo_ntt import NTTClient
    assert callable(NTTClient.vec_horner) and callable(NTTClient.vec_divide)
    assert (NTTClient.HORNER_EXCLUSIVE, NTTClient.HORNER_REVERSE) == (1, 2)
    assert "_vec_keep" in NTTClient.vec_horner.__code__.co_names and "_vec_keep" in NTTClient.vec_divide.__code__.co_names
    hpp = _read("include", "blaze.hpp")
    assert "blz_ntt_vec_horner(" in hpp and re.search(r"void\s+vec_horner\s*\(", hpp) and re.search(r"void\s+vec_divide\s*\(", hpp)
    assert "pub fn blz_ntt_vec_horner" in _read("rust", "src", "driver_client", "hip_ffi.rs")
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "fn vec_horner" in api and "fn vec_divide" in api and "blz_ntt_vec_horner(" in api
    # the kernels live in their own header and reach the handle through NttFieldOps
    assert '#include "ntt_horner.hip.hpp"' in _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    assert re.search(r"\(\*vec_horner\)\s*\(", _read("blaze_amd", "csrc", "ntt_engine.hpp"))
    assert "o.vec_horner" in _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    return kernel_vgprs(LIB), kernel_scratch(LIB)


def test_horner_kernels_stay_out_of_scratch_and_within_128_vgprs(code):
    vgprs, scratch = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_horner_", n))
    print({n: (vgprs[n], scratch[n]) for n in names})
    per_field = [[n for n in names if re.match(rf"_ZN3blz\d+k_horner_\w+?INS_{f}E", n)] for f in FIELDS]
    assert per_field[0] and len({len(p) for p in per_field}) == 1, per_field
    assert sum(len(p) for p in per_field) == len(names), names    # instantiated on the three scalar fields and nothing else
    # the same kernels for every field
    assert len({tuple(re.sub(r"INS_\d+Fr_[A-Z0-9]+E", "", n) for n in p) for p in per_field}) == 1, per_field
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= 128, (n, vgprs[n])
        # the other ISA tests select kernels by these fragments: the new ones stay out of their sets
        assert not re.match(r"_ZN3blz\d+k_fold_", n) and not re.match(r"_ZN3blz\d+k_vec_", n) and not re.match(r"_ZN3blz\d+k3t?_", n)
        assert "k_ntt512_rr" not in n and "poseidon" not in n
