"""Scatter-add on resident buffers (blz_ntt_vec_scatter), the part that needs no device: the entry point and the 40-byte struct
exist in every layer with the documented signature, field order and position (gather - scatter - spmv), a null handle is refused
whatever else is passed, the entry point reaches the kernels through NttFieldOps once and copies no pointer check, and the
shipped gfx950 code object holds what the kernels promise - every k_scatter_* kernel exists for the three scalar fields and
nothing else, the same set per field, stays out of scratch and within 128 VGPRs, falls into no kernel family another ISA test
counts, the accumulating kernels add with 64-bit global atomics and hold no compare-and-swap, the finishing kernels hold no
atomic at all and the histogram no multiply."""
import ctypes
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, count, disassemble_library, function_instructions, kernel_scratch, kernel_vgprs, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

NAME = "blz_ntt_vec_scatter"
FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
SCATTER_FIELDS = ("d_idx", "d_src", "d_val", "nnz", "reserved")


def test_declaration_and_struct_in_the_header():
    hdr = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+blz_ntt_vec_scatter\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*size_t\s+buf_dst\s*,\s*const\s+blz_vec_arg\s*\*\s*x\s*,"
                     r"\s*const\s+blz_vec_scatter\s*\*\s*s\s*\)\s*;", code)
    m = re.search(r"typedef\s+struct\s+blz_vec_scatter\s*\{\s*const\s+uint32_t\s*\*\s*d_idx\s*;\s*const\s+uint32_t\s*\*\s*d_src\s*;"
                  r"\s*const\s+void\s*\*\s*d_val\s*;\s*uint64_t\s+nnz\s*;\s*uint64_t\s+reserved\s*;\s*\}\s*blz_vec_scatter\s*;", code)
    assert m   # three pointers and two 64-bit words: 40 bytes, no padding
    # the header reads gather, scatter, spmv: the comment, the struct and the declaration between the two
    assert code.index("blz_ntt_vec_gather(") < code.index("typedef struct blz_vec_scatter") < code.index(NAME + "(") < code.index("typedef struct blz_vec_csr")
    assert hdr.index("blz_ntt_vec_gather(blz_ntt") < hdr.index("Scatter-add on resident buffers") < hdr.index("typedef struct blz_vec_scatter")
    assert hdr.index(NAME + "(blz_ntt") < hdr.index("Sparse matrix-vector products on resident buffers")
    assert re.search(r"\}\s*blz_vec_scatter;\s*/\* 40 bytes \*/", hdr)
    contract = hdr[hdr.index("Scatter-add on resident buffers"):hdr.index("typedef struct blz_vec_scatter")]
    for words in ("histogram", "canonical", "same bytes", "2^31", "reserved != 0", "d_src given without x", "null handle", "blz_ntt_wait_result",
                  "may NOT name buf_dst", "2^27"):
        assert words in contract, words


def test_binding_table_and_struct_mirror():
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzVecArg, BlzVecScatter
    assert EXPORTED_SYMBOLS.index("blz_ntt_vec_gather") < EXPORTED_SYMBOLS.index(NAME) < EXPORTED_SYMBOLS.index("blz_ntt_vec_spmv")
    assert EXPORTED_SYMBOLS.index(NAME) == EXPORTED_SYMBOLS.index("blz_ntt_vec_gather") + 1
    assert _SIGS[NAME] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(BlzVecArg), ctypes.POINTER(BlzVecScatter)])
    assert getattr(ctypes.CDLL(LIB), NAME) is not None
    assert [n for n, _ in BlzVecScatter._fields_] == list(SCATTER_FIELDS)
    assert [t for _, t in BlzVecScatter._fields_] == [ctypes.c_void_p] * 3 + [ctypes.c_uint64] * 2
    assert ctypes.sizeof(BlzVecScatter) == 40
    assert [getattr(BlzVecScatter, f).offset for f in SCATTER_FIELDS] == [0, 8, 16, 24, 32]


def test_null_handle_is_refused_before_anything_else_is_looked_at():
    from blaze_amd._lib import BlzVecArg, BlzVecScatter
    L = blaze_amd.lib()
    x, s = BlzVecArg(None, 0, 0, 0), BlzVecScatter(None, None, None, 0, 0)
    assert L.blz_ntt_vec_scatter(None, 0, ctypes.byref(x), ctypes.byref(s)) == 4
    assert L.blz_ntt_vec_scatter(None, 99, None, None) == 4
    assert L.blz_ntt_vec_scatter(None, 7, ctypes.byref(BlzVecArg(8, 7, 1, 3)), ctypes.byref(BlzVecScatter(2, 6, 4, 1 << 50, 9))) == 4
    L.blz_last_error_message.restype = ctypes.c_char_p
    assert b"null handle" in L.blz_last_error_message()


def test_mirrors_and_documents():
    from blaze_amd.ingo_ntt import NTTClient
    for f in (NTTClient.vec_scatter, NTTClient.vec_count):
        assert callable(f) and "_vec_keep" in f.__code__.co_names, f
    assert NTTClient.vec_scatter.__code__.co_varnames[:7] == ("self", "dst", "idx", "x", "val", "src", "nnz")
    assert NTTClient.vec_scatter.__defaults__ == (None, None, None, None)
    assert NTTClient.vec_count.__code__.co_varnames[:4] == ("self", "dst", "idx", "nnz")
    assert NTTClient.vec_count.__defaults__ == (None,)
    hpp = _read("include", "blaze.hpp")
    assert "blz_ntt_vec_scatter(" in hpp and "blz_vec_scatter" in hpp
    for f in ("vec_scatter", "vec_count"):
        assert re.search(rf"void\s+{f}\s*\(", hpp), f
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_vec_scatter\(h: \*mut BlzNtt, buf_dst: usize, x: \*const BlzVecArg, s: \*const BlzVecScatter\) -> c_int;", ffi)
    assert re.search(r"#\[repr\(C\)\]\s*(#\[derive\([^\]]*\)\]\s*)?pub struct BlzVecScatter\s*\{\s*pub d_idx: \*const u32,\s*pub d_src: \*const u32,"
                     r"\s*pub d_val: \*const c_void,\s*pub nnz: u64,\s*pub reserved: u64,?\s*\}", ffi)
    assert ffi.index("pub fn blz_ntt_vec_gather(") < ffi.index("pub fn blz_ntt_vec_scatter(") < ffi.index("pub fn blz_ntt_vec_spmv(")
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "pub unsafe fn vec_scatter(" in api and "pub unsafe fn vec_count(" in api and "blz_ntt_vec_scatter(" in api
    assert re.search(r"BlzVecScatter\s*\{\s*d_idx\s*,\s*d_src\s*,\s*d_val\s*,\s*nnz\s*,\s*reserved:\s*0\s*\}", api)   # by name: the order is the struct's
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md"):
        assert "vec_scatter" in _read(doc), doc
    assert "Scatter-add" in _read("DESIGN.md")


def test_host_side_is_one_entry_point_on_the_shared_protocol():
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.count("h->ops->vec_scatter(") == 1
    body = ntt[ntt.index("int blz_ntt_vec_scatter("):ntt.index("// Multilinear tables (ntt_mle.hip.hpp)")]
    assert "h->ops->vec_scatter(" in body and ntt.index("int blz_ntt_vec_spmv(") < ntt.index("int blz_ntt_vec_scatter(")
    for step in ("NttVecCall call{h}", "call.begin()", "call.resolve(", "call.enqueue("):
        assert step in body, step
    assert all(re.search(rf'device_range\("[^"]*",\s*"{f}"', body) for f in SCATTER_FIELDS[:3]), body
    assert body.index('"null handle"') < body.index("s->") and body.index('"null handle"') < body.index("buf_dst >")
    # the helpers are used, not copied
    assert ntt.count("hipMemGetAddressRange(") == 1 and ntt.count("hipPointerGetAttributes(&at") == 1 and ntt.count("is not a power of two") == 1
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    assert '#include "ntt_scatter.hip.hpp"' in impl and "o.vec_scatter = &ntt_vec_scatter_t<Fr>" in impl
    assert re.search(r"\(\*vec_scatter\)\s*\(\s*hipStream_t\s+st\s*,\s*uint32_t\s*\*\s*dst\s*,\s*NttVecArg\s+x\s*,\s*const\s+uint32_t\s*\*\s*idx\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*src\s*,\s*const\s+uint32_t\s*\*\s*val\s*,\s*uint64_t\s+nnz\s*,\s*uint64_t\s+n\s*,\s*uint32_t\s*\*\s*ws\s*\)",
                     _read("blaze_amd", "csrc", "ntt_engine.hpp"))
    src = _read("blaze_amd", "csrc", "ntt_scatter.hip.hpp")
    for banned in ("volatile", "alloc", "asm"):
        assert banned not in src, banned
    assert "__hip_atomic_fetch_add" in src and "__ATOMIC_RELAXED" in src and "__HIP_MEMORY_SCOPE_AGENT" in src
    assert "hipMemsetAsync" in src   # the dispatch zeroes what the mode accumulates into
    # the thresholds are within the ceilings: n x 64 and n x 4 bytes of a block's 64 KiB
    lds_add, lds_count = (int(re.search(rf"constexpr uint64_t {c} = (\d+);", src).group(1)) for c in ("SCATTER_LDS_ADD", "SCATTER_LDS_COUNT"))
    assert lds_add <= 1024 and lds_count <= 16384 and lds_add & (lds_add - 1) == 0 and lds_count & (lds_count - 1) == 0


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    return kernel_vgprs(LIB), kernel_scratch(LIB), disassemble_library(LIB)


def _scatter_kernels(vgprs):
    return sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_scatter_", n))


def test_scatter_kernels_stay_out_of_scratch_and_within_128_vgprs(code):
    vgprs, scratch, _ = code
    names = _scatter_kernels(vgprs)
    print({n: (vgprs[n], scratch[n]) for n in names})
    per_field = [[n for n in names if re.match(rf"_ZN3blz\d+k_scatter_\w+?INS_{f}E", n)] for f in FIELDS]
    # add and its LDS twin in the three combinations of x and val, the finish, and the histogram's three
    assert len(per_field[0]) == 10 and len({len(p) for p in per_field}) == 1, per_field
    assert sum(len(p) for p in per_field) == len(names), names    # instantiated on the three scalar fields and nothing else
    assert len({tuple(re.sub(r"INS_\d+Fr_[A-Z0-9]+E", "", n) for n in p) for p in per_field}) == 1, per_field   # the same set per field
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= 128, (n, vgprs[n])
        # the other ISA tests select kernels by these fragments: the new ones stay out of their sets
        for family in (r"k_sc_", r"k_spmv_", r"k_gather_", r"k_vec_", r"k_fold_", r"k_mle_", r"k_horner_", r"k_gate_", r"k3t?_"):
            assert not re.match(rf"_ZN3blz\d+{family}", n), (n, family)
        assert "k_ntt512_rr" not in n and "poseidon" not in n


def test_atomics_per_kernel(code):
    """The accumulating kernels add with return-less 64-bit global atomics and never loop on a compare-and-swap; a finishing
    kernel holds no atomic of any kind (its position is its lane's alone); the histogram needs no multiplier - v_mad_u64_u32 is
    the multiplier of field.hip.hpp, and index arithmetic that needed one would show here too."""
    vgprs, _, text = code
    names = _scatter_kernels(vgprs)
    ops = {n: [o for _, o, _ in function_instructions(text, n)] for n in names}
    kind = lambda n: re.match(r"_ZN3blz\d+(k_scatter_[a-z_]+?)I", n).group(1)   # noqa: E731
    assert {kind(n) for n in names} == {"k_scatter_add", "k_scatter_add_lds", "k_scatter_fin", "k_scatter_count", "k_scatter_count_lds", "k_scatter_count_fin"}
    for n in names:
        atomics = [o for o in ops[n] if "atomic" in o or re.match(r"ds_(add|cmpst|inc|wrxchg)", o)]
        print(n, sorted(set(atomics)), count(function_instructions(text, n), "v_mad_u64_u32"))
        assert not any("cmpswap" in o or "cmpst" in o for o in ops[n]), n
        if kind(n) in ("k_scatter_add", "k_scatter_add_lds"):
            assert "global_atomic_add_x2" in atomics, (n, atomics)
            assert not any(o.endswith("_rtn") or "_rtn_" in o for o in atomics), (n, atomics)
        if kind(n) == "k_scatter_add_lds":
            assert "ds_add_u64" in atomics, (n, atomics)
        if kind(n) in ("k_scatter_fin", "k_scatter_count_fin"):
            assert atomics == [], (n, atomics)
        if kind(n) in ("k_scatter_count", "k_scatter_count_lds"):
            assert "global_atomic_add" in atomics and "v_mad_u64_u32" not in ops[n], (n, atomics)
        if kind(n) == "k_scatter_count_lds":
            assert "ds_add_u32" in atomics, (n, atomics)
    # the product is taken where both operands are present and nowhere else: two Montgomery products of 128 multiplies
    for f in FIELDS:
        mads = {(b1, b2): count(function_instructions(text, next(n for n in names if re.match(rf"_ZN3blz\d+k_scatter_addINS_{f}ELb{b1}ELb{b2}E", n))), "v_mad_u64_u32")
                for b1, b2 in ((1, 1), (1, 0), (0, 1))}
        assert mads[(1, 1)] >= 128 > mads[(1, 0)] and mads[(0, 1)] < 128, (f, mads)
