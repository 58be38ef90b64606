"""Coset transforms (blz_ntt_set_coset), the part that needs no device: the entry points exist in every layer, and the coset
instantiations of the 512-point kernel hold what "fused" means in numbers - measured on the shipped gfx950 code object, each
against its plain sibling in the same disassembly (BLS12-381 Fr):
  * a forward handle's wire pass (pass 1 at 2^27, pass 2 at 2^18) holds one more Shoup product per element: 8 x 143 multiply-adds,
    and at most four per-lane set-up products;
  * every other coset instantiation - pass 2 above 2^18 with its stepped factor, pass 3 of an inverse handle - holds per-lane
    set-up only: no per-element product.  (Pass 2 with the per-element factor table has no coset instantiation: the handle folds
    the shift into the table's entries and launches the plain kernel.)
  * every coset kernel stays within three blocks per CU (168 VGPRs) and out of scratch."""
import ctypes
import os
import re

import pytest

import blaze_amd
from isa_util import count, disassemble_library, function_instructions, kernel_vgprs, tools_available

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

PLAIN = "_ZN3blz11k_ntt512_rrINS_9Fr_BLS381ELi{p}ELb{tab}EEEvPKjPjNS_7NttGeomENS_11NttTablesRRE"
COSET = "_ZN3blz14k_ntt512_rr_csINS_9Fr_BLS381ELi{p}ELi{cs}EEEvPKjPjNS_7NttGeomENS_11NttTablesRRENS_8NttCosetE"
TOL = 8   # test_isa_counts.py's tolerance


def test_entry_points_in_every_layer():
    hdr = open(os.path.join(ROOT, "include", "blaze_hip.h")).read()
    assert re.search(r"int\s+blz_ntt_set_coset\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*const\s+uint8_t\s*\*\s*shift\s*\)\s*;", hdr)
    assert re.search(r"int\s+blz_ntt_get_coset\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*uint8_t\s+out\[32\]\s*\)\s*;", hdr)
    from blaze_amd._lib import EXPORTED_SYMBOLS
    raw = ctypes.CDLL(LIB)
    for name in ("blz_ntt_set_coset", "blz_ntt_get_coset"):
        assert name in EXPORTED_SYMBOLS
        assert getattr(raw, name) is not None
    L = blaze_amd.lib()
    one = (1).to_bytes(32, "little")
    assert L.blz_ntt_set_coset(None, None) == 4
    assert L.blz_ntt_set_coset(None, ctypes.cast(ctypes.c_char_p(one), ctypes.c_void_p)) == 4
    out = ctypes.create_string_buffer(32)
    assert L.blz_ntt_get_coset(None, ctypes.cast(out, ctypes.c_void_p)) == 4
    # the mirrors
    from blaze_amd.ingo_ntt import NTTClient
    assert callable(NTTClient.set_coset) and isinstance(NTTClient.coset, property)
    assert "blz_ntt_set_coset" in open(os.path.join(ROOT, "include", "blaze.hpp")).read()
    assert "blz_ntt_set_coset" in open(os.path.join(ROOT, "rust", "src", "driver_client", "hip_ffi.rs")).read()
    assert "fn set_coset" in open(os.path.join(ROOT, "rust", "src", "ingo_ntt", "ntt_api.rs")).read()


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    text = disassemble_library(LIB)
    notes = disassemble_library(LIB, "llvm-readelf", "--notes")
    scratch = {n: int(v) for n, v in re.findall(
        r"^\s+\.name:\s+(\S+)\n(?:(?!\s+\.name:).*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", notes, re.M)}
    return text, kernel_vgprs(LIB), scratch


def _mads(text, name):
    return count(function_instructions(text, name), "v_mad_u64_u32")


def test_plain_kernels_keep_their_names(code):
    text, vgprs, _ = code
    for p, tab in ((1, 0), (2, 0), (2, 1), (3, 0)):
        assert PLAIN.format(p=p, tab=tab) in vgprs
        assert _mads(text, PLAIN.format(p=p, tab=tab)) > 0
    for p in (1, 2, 3):
        assert f"_ZN3blz10k_ntt_passINS_9Fr_BLS381ELi{p}EEEvPKjPjNS_7NttGeomENS_9NttTablesEi" in vgprs


@pytest.mark.parametrize("p", [1, 2])
def test_wire_pass_holds_one_product_per_element(code, p):
    """pass 1 (2^27) and pass 2 as run at 2^18: eight elements per lane, one Shoup product each (143 multiply-adds; 153 were it a
    Montgomery one), up to four per-lane set-up products."""
    text, _, _ = code
    extra = _mads(text, COSET.format(p=p, cs=1)) - _mads(text, PLAIN.format(p=p, tab=0))
    print(f"pass {p} wire: + {extra} multiply-adds")
    assert 8 * 143 - TOL <= extra <= 8 * 153 + 4 * 153 + TOL, extra


@pytest.mark.parametrize("p,cs", [(2, 2), (3, 3)])
def test_other_passes_hold_no_product_per_element(code, p, cs):
    """pass 2 above 2^18 (stepped factor: the start value takes the folded part, the step is a rebuilt table's) and pass 3 of an
    inverse handle (the closing factor is read by row instead of held): per-lane set-up only."""
    text, _, _ = code
    plain, coset = _mads(text, PLAIN.format(p=p, tab=0)), _mads(text, COSET.format(p=p, cs=cs))
    print(f"pass {p} coset variant {cs}: {coset} multiply-adds, plain {plain}")
    assert coset <= plain + 4 * 153 + TOL, (coset, plain)


def test_coset_kernels_keep_three_blocks_per_cu(code):
    _, vgprs, scratch = code
    names = [n for n in vgprs if re.match(r"_ZN3blz14k_ntt512_rr_csI", n)]
    # 4 variants x 3 fields, and nothing else: a pass-2 kernel on the factor table would be the plain one again
    assert len(names) == 12 and {COSET.format(p=p, cs=cs) for p, cs in ((1, 1), (2, 1), (2, 2), (3, 3))} <= set(names), sorted(names)
    for n in names:
        assert vgprs[n] <= 168, (n, vgprs[n])
        assert scratch[n] == 0, (n, scratch[n])
