"""Element-wise ops on resident buffers (blz_ntt_vec_op), the part that needs no device: the entry point and its operand struct
exist in every layer, and the shipped gfx950 code object holds what the kernels promise - every k_vec_* kernel of the three
fields stays out of scratch and within 128 VGPRs (four waves per SIMD), and the loop of the element-wise product holds the
multiply-adds of two field products, not three.  One product's figure is read from the same code object: the loop of
k_ntt_ninv<Fr> is one fp_mul and nothing else."""
import ctypes
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, count, disassemble_library, function_instructions, kernel_scratch, kernel_vgprs, loops, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
EW = "_ZN3blz8k_vec_ewINS_{f}ELi{op}EEEvPjNS_9NttVecArgES3_S3_m"
NINV = "_ZN3blz10k_ntt_ninvINS_{f}EEEvPji"
TOL = 8   # test_isa_counts.py's tolerance


def test_entry_point_and_struct_in_every_layer():
    hdr = _read("include", "blaze_hip.h")
    assert re.search(r"int\s+blz_ntt_vec_op\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*int\s+op\s*,\s*size_t\s+buf_dst\s*,\s*const\s+blz_vec_arg\s*\*\s*a\s*,"
                     r"\s*const\s+blz_vec_arg\s*\*\s*b\s*,\s*const\s+blz_vec_arg\s*\*\s*c\s*\)\s*;", hdr)
    m = re.search(r"typedef\s+struct\s+blz_vec_arg\s*\{(.*?)\}\s*blz_vec_arg\s*;", hdr, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == ["d_ptr", "buf", "reserved", "count"]
    for k, name in enumerate(("ADD", "SUB", "MUL", "MULADD", "MULSUB", "INV")):
        assert re.search(rf"BLZ_VEC_{name}\s*=\s*{k}\b", hdr), name
    assert "POSITION" in hdr[hdr.index("Element-wise ops"): hdr.index("enum blz_vec_op")]   # the period runs along positions: said so
    from blaze_amd._lib import EXPORTED_SYMBOLS, BlzVecArg
    assert "blz_ntt_vec_op" in EXPORTED_SYMBOLS
    assert getattr(ctypes.CDLL(LIB), "blz_ntt_vec_op") is not None
    assert [f[0] for f in BlzVecArg._fields_] == ["d_ptr", "buf", "reserved", "count"]
    assert ctypes.sizeof(BlzVecArg) == 24 and BlzVecArg.count.offset == 16 and BlzVecArg.buf.offset == 8
    # a null handle is refused before anything else is looked at
    L = blaze_amd.lib()
    a = BlzVecArg(None, 0, 0, 0)
    assert L.blz_ntt_vec_op(None, 2, 0, ctypes.byref(a), ctypes.byref(a), None) == 4
    assert L.blz_ntt_vec_op(None, 0, 0, None, None, None) == 4
    # the mirrors
    from blaze_amd import ingo_ntt
    from blaze_amd.ingo_ntt import NTTClient
    assert callable(NTTClient.vec_op) and callable(NTTClient.scalar)
    assert [NTTClient.ADD, NTTClient.SUB, NTTClient.MUL, NTTClient.MULADD, NTTClient.MULSUB, NTTClient.INV] == list(range(6))
    tile = re.search(r"NTT_VEC_INV_TILE\s*=\s*(\d+)\s*;", _read("blaze_amd", "csrc", "ntt_engine.hpp"))
    assert tile and ingo_ntt.VEC_INV_TILE == int(tile.group(1))
    hpp = _read("include", "blaze.hpp")
    assert "blz_ntt_vec_op" in hpp and re.search(r"void\s+vec_op\s*\(", hpp)
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert "pub fn blz_ntt_vec_op" in ffi
    rs = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^)]*\)\]\s*)?pub struct BlzVecArg\s*\{(.*?)\}", ffi, re.S)
    assert rs and re.findall(r"pub (\w+)\s*:", rs.group(1)) == ["d_ptr", "buf", "reserved", "count"]
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "fn vec_op" in api and "blz_ntt_vec_op(" in api


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    text = disassemble_library(LIB)
    return text, kernel_vgprs(LIB), kernel_scratch(LIB)


def test_vec_kernels_stay_out_of_scratch_and_within_128_vgprs(code):
    _, vgprs, scratch = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_vec_", n))
    print({n: (vgprs[n], scratch[n]) for n in names})
    # per field: the five arithmetic instantiations and the inversion's three kernels
    assert len(names) == 3 * 8, names
    for f in FIELDS:
        assert {EW.format(f=f, op=op) for op in range(5)} <= set(names)
        for stem in ("k_vec_inv_up", "k_vec_inv_mid", "k_vec_inv_down"):
            assert any(stem in n and f in n for n in names), (stem, f)
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= 128, (n, vgprs[n])
        # the existing ISA tests select kernels by these fragments: the new ones stay out of their sets
        assert not re.match(r"_ZN3blz\d+k3t?_", n) and "k_ntt512_rr" not in n and "poseidon" not in n


@pytest.mark.parametrize("f", FIELDS)
def test_product_loop_holds_two_field_products(code, f):
    text, _, _ = code
    one = [count(body, "v_mad_u64_u32") for _, _, body in loops(function_instructions(text, NINV.format(f=f)))]
    assert len(one) == 1 and one[0] >= 8 * 8 * 2, one   # the loop of k_ntt_ninv: acc = acc * two, one fp_mul (>= N^2 for a b and for q m)
    one = one[0]
    body = [count(b, "v_mad_u64_u32") for _, _, b in loops(function_instructions(text, EW.format(f=f, op=2)))]
    print(f"{f}: one product {one} multiply-adds, the MUL kernel's loops {body}")
    assert len(body) == 1, body                               # the grid-stride loop, nothing else
    assert abs(body[0] - 2 * one) <= TOL, (body, one)
    assert body[0] < 3 * one - TOL
    # the whole kernel is that loop: no product outside it
    assert count(function_instructions(text, EW.format(f=f, op=2)), "v_mad_u64_u32") == body[0]
