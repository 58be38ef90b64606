"""Product and fraction trees (blz_ntt_mle_tree), the part that needs no device: the entry point exists in every layer with the
signature the header gives and at the places the other tests leave free, a null handle is refused whatever else is passed, the
Python client's signature and layer arithmetic, DeviceBuffer.view, the kernels live in their own header behind one NttFieldOps
slot, the documents speak of the op, and the shipped gfx950 code object holds what the kernels promise - eight k_tree_ kernels
per scalar field, no scratch, VGPRs within the family's bound, the products inlined."""
import ctypes
import inspect
import os
import re

import pytest

import blaze_amd
from isa_util import ROOT, _read, count, disassemble_library, function_body, function_instructions, kernel_scratch, kernel_vgprs, tools_available

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
NAME = "blz_ntt_mle_tree"
# the fragments the other ISA tests select their kernels by
FAMILIES = (r"k_gate_", r"k_vec_", r"k_sc_", r"k_mle_", r"k_fold_", r"k_horner_", r"k_gather_", r"k_spmv_", r"k_scatter_", r"k3", r"k_geval", r"k_lineval",
            r"k_zc_", r"k_ntt512_rr")


def _uncommented(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_declared_in_the_header_between_sumcheck_gate_and_gate_eval():
    raw = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    arg = r"const\s+blz_vec_arg\s*\*\s*"
    assert re.search(rf"int\s+{NAME}\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*uint32_t\s+op\s*,\s*uint32_t\s+flags\s*,\s*{arg}dst\s*,\s*{arg}dst_q\s*,\s*{arg}a\s*,"
                     rf"\s*{arg}a_q\s*,\s*uint64_t\s+len\s*\)\s*;", code)
    assert re.search(r"enum\s+blz_tree_op\s*\{\s*BLZ_TREE_PROD\s*=\s*0\s*,\s*BLZ_TREE_FRAC\s*=\s*1\s*\}\s*;", code)
    assert code.index("blz_ntt_sumcheck_gate(") < code.index(NAME + "(") < code.index("blz_ntt_gate_eval(")
    # nothing else is declared between the gate step and the trees, nor between the trees and the evaluation
    assert not re.search(r"\bblz_[a-z0-9_]+\s*\(", code[code.index("blz_ntt_sumcheck_gate(") + 25: code.index(NAME + "(")])
    assert not re.search(r"\bblz_[a-z0-9_]+\s*\(", code[code.index(NAME + "(") + len(NAME) + 1: code.index("blz_ntt_gate_eval(")])
    # ahead of the comment of blz_ntt_gate_eval, which still stands directly in front of its declaration
    assert raw.index(NAME + "(blz_ntt* h") < raw.index("/* The same description evaluated POSITION BY POSITION") < raw.index("int blz_ntt_gate_eval(")
    assert not NAME.startswith("blz_ntt_vec_")


def test_defined_where_no_other_tests_slice_covers_it():
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    at = ntt.index(f"int {NAME}(")
    assert ntt.index("int blz_ntt_gate_eval_lin(") < at < ntt.index("int blz_ntt_last_kernel_ms(")
    assert not ntt.index("int blz_ntt_vec_mle_fold(") < at < ntt.index("int blz_ntt_stream(")
    assert ntt.count(f"int {NAME}(") == 1


def test_exported_and_bound():
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzVecArg
    assert NAME in EXPORTED_SYMBOLS
    assert EXPORTED_SYMBOLS.index(NAME) == EXPORTED_SYMBOLS.index("blz_ntt_zerocheck_gate") + 1
    P = ctypes.POINTER(BlzVecArg)
    assert _SIGS[NAME] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, P, P, P, P, ctypes.c_uint64])
    assert getattr(ctypes.CDLL(LIB), NAME) is not None


def test_null_handle_is_refused_before_anything_else_is_looked_at():
    from blaze_amd._lib import BlzVecArg
    L = blaze_amd.lib()
    v, bad = BlzVecArg(None, 0, 0, 0), BlzVecArg(8, 7, 1, 3)
    r = ctypes.byref
    for args in ((0, 0, r(v), None, r(v), None, 4), (1, 1, r(v), r(v), r(v), r(v), 8), (99, 0xFFFFFFFF, r(bad), r(bad), r(bad), r(bad), 1 << 60),
                 (0, 0, None, None, None, None, 0), (1, 2, None, r(bad), r(v), None, 3), (7, 0, r(v), None, None, r(bad), 0xFFFFFFFFFFFFFFFF)):
        assert getattr(L, NAME)(None, *args) == 4
        assert b"null handle" in L.blz_last_error_message()


def test_python_client_signature():
    from blaze_amd.ingo_ntt import NTTClient
    assert (NTTClient.TREE_PROD, NTTClient.TREE_FRAC) == (0, 1)
    f = NTTClient.mle_tree
    assert callable(f) and "_vec_keep" in f.__code__.co_names and NAME in f.__code__.co_names
    sig = inspect.signature(f)
    assert list(sig.parameters) == ["self", "dst", "a", "op", "length", "low", "dst_q", "a_q"]
    assert [sig.parameters[p].default for p in ("op", "length", "low", "dst_q", "a_q")] == [NTTClient.TREE_PROD, None, False, None, None]
    assert all(sig.parameters[p].default is inspect.Parameter.empty for p in ("dst", "a"))


def test_tree_layer_against_the_formula():
    from blaze_amd.ingo_ntt import NTTClient
    assert isinstance(inspect.getattr_static(NTTClient, "tree_layer"), staticmethod)
    assert NTTClient.tree_layer(2, 1) == (0, 1)
    assert [NTTClient.tree_layer(8, k) for k in (1, 2, 3)] == [(0, 4), (4, 2), (6, 1)]
    for length in (2, 8, 1 << 27):
        m = length.bit_length() - 1
        layers = [NTTClient.tree_layer(length, k) for k in range(1, m + 1)]
        assert layers == [(length - length // 2 ** (k - 1), length // 2 ** k) for k in range(1, m + 1)]
        # back to back from word 0, length - 1 words in all, the root at length - 2
        assert layers[0][0] == 0 and layers[-1] == (length - 2, 1)
        assert all(layers[i][0] + layers[i][1] == layers[i + 1][0] for i in range(m - 1))
        assert sum(w for _, w in layers) == length - 1
        for k in (0, m + 1):
            with pytest.raises(ValueError):
                NTTClient.tree_layer(length, k)
    for length in (0, 1, 3, 12):
        with pytest.raises(ValueError):
            NTTClient.tree_layer(length, 1)


def test_device_buffer_view():
    from blaze_amd import DeviceBuffer
    from blaze_amd.ingo_ntt import NTTClient
    assert callable(DeviceBuffer.view)
    assert list(inspect.signature(DeviceBuffer.view).parameters) == ["self", "offset_bytes", "nbytes"]
    # no device: a parent built by hand
    parent = DeviceBuffer.__new__(DeviceBuffer)
    parent.device_id, parent.nbytes, parent.ptr = 0, 1024, 0x10000
    v = parent.view(64, 256)
    assert isinstance(v, DeviceBuffer) and type(v) is not DeviceBuffer
    assert (v.ptr, v.nbytes, v.device_id) == (0x10000 + 64, 256, 0) and v.parent is parent
    arg = NTTClient._vec_arg(v)
    assert (arg.d_ptr, arg.count) == (0x10000 + 64, 8)
    v.free()
    assert v.ptr == 0x10000 + 64 and parent.ptr == 0x10000   # a view frees nothing
    w = v.view(32, 32)   # a view of a view keeps the chain alive
    assert w.ptr == 0x10000 + 96 and w.parent is v
    for off, nb in ((-1, 8), (0, 1025), (1000, 32), (0, -1)):
        with pytest.raises(ValueError):
            parent.view(off, nb)
    parent.ptr = None   # nothing for __del__ to free


def test_mirrors():
    hpp = _read("include", "blaze.hpp")
    assert NAME + "(" in hpp and re.search(r"void\s+mle_tree\s*\(\s*uint32_t\s+op\s*,", hpp) and "tree_layer(" in hpp
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_mle_tree\(h: \*mut BlzNtt, op: u32, flags: u32, dst: \*const BlzVecArg, dst_q: \*const BlzVecArg, a: \*const BlzVecArg,"
                     r"\s*a_q: \*const BlzVecArg,\s*len: u64\) -> c_int;", ffi)
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "pub unsafe fn mle_tree(" in api and NAME + "(" in api and "pub fn tree_layer(" in api and "pub enum TreeOp" in api


def test_kernels_in_their_own_header_behind_one_slot():
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    eng = _read("blaze_amd", "csrc", "ntt_engine.hpp")
    assert impl.index('#include "ntt_lineval.hip.hpp"') < impl.index('#include "ntt_tree.hip.hpp"')
    assert impl.count("o.mle_tree = ") == 1 and len(re.findall(r"\(\*mle_tree\)\s*\(\s*hipStream_t\s+st\s*,", eng)) == 1
    src = _read("blaze_amd", "csrc", "ntt_tree.hip.hpp")
    kernels = re.findall(r"template\s*<([^>]*)>\s*__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", src)
    assert kernels == [("class Fr, int OP, bool LOW", "k_tree_up"), ("class Fr, int OP, bool LOW", "k_tree_top")], kernels
    statements = _uncommented(src)
    for banned in ("atomic", "alloc", "volatile", "__threadfence", "ws"):
        assert not re.search(rf"\b{banned}", statements), banned
    # every lane of the one block reaches every barrier: nothing returns out of the kernels
    body = statements[statements.index("void k_tree_up("): statements.index("int ntt_mle_tree_launch(")]
    assert "return" not in body and body.count("__syncthreads()") == 3
    # no kernel of the neighbouring families moved in or out
    assert "k_mle_" not in statements
    assert re.findall(r"__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", _read("blaze_amd", "csrc", "ntt_mle.hip.hpp")) == ["k_mle_fold", "k_mle_eq"]


def test_entry_point_walks_the_shared_protocol():
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    body = function_body(ntt, f"int {NAME}(")
    for once in ("call.destination(", "call.resolve(", "call.enqueue(", "call.begin()", "call.live_length(", "h->ops->mle_tree("):
        assert body.count(once) == 1, once
    for elsewhere in ("hipPointerGetAttributes", "hipMemGetAddressRange", "device_range(", "hipMemcpy"):
        assert elsewhere not in body, elsewhere
    assert body.index('"null handle"') < body.index("unknown tree op") < body.index("unknown multilinear flags") < body.index("call.live_length(") \
        < body.index("call.begin()") < body.index("call.resolve(") < body.index("call.destination(") < body.index("call.enqueue(")
    assert ntt.count("h->ops->mle_tree(") == 1


def test_documented_where_the_other_ops_are():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md"):
        assert "mle_tree" in _read(doc), doc
    design = _read("DESIGN.md")
    assert "Product and fraction trees" in design and "k_tree_up" in design and "k_tree_top" in design
    assert "ntt_tree_timing.py" in design and "ntt_tree_ops.json" in design


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    return kernel_vgprs(LIB), kernel_scratch(LIB), disassemble_library(LIB)


VGPR_CAP = 128   # the family's bound: four waves of 256 lanes per SIMD ("Product and fraction trees")


def test_eight_kernels_per_field_without_scratch_within_128_vgprs(code):
    vgprs, scratch, text = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_tree_", n))
    print({n: (vgprs[n], scratch[n]) for n in names})
    assert len(names) == 24, names
    per_field = [sorted(n.replace(f, "F") for n in names if re.match(rf"_ZN3blz\d+k_tree_\w+?INS_{f}E", n)) for f in FIELDS]
    assert all(len(p) == 8 for p in per_field), per_field
    assert per_field[0] == per_field[1] == per_field[2]
    # 2 ops x 2 pairings x 2 kernels
    for kernel, tail in (("9k_tree_up", "mm"), ("10k_tree_top", "jm")):
        for op in (0, 1):
            for low in (0, 1):
                want = f"_ZN3blz{kernel}INS_FELi{op}ELb{low}EEEvNS_7TreeDstENS_7TreeSrcE{tail}"
                assert want in per_field[0], (want, per_field[0])
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= VGPR_CAP, (n, vgprs[n])
        # a node is two products (PROD) or five (FRAC), inlined: 2 x 64 multiply-adds per product of 8 x 8 limbs with its reduction
        assert count(function_instructions(text, n), "v_mad_u64_u32") >= 256, n
        for family in FAMILIES:
            assert not re.match(rf"_ZN3blz\d+{family}", n), (n, family)
        assert "poseidon" not in n
    # the neighbours keep their counts
    assert len([n for n in vgprs if re.match(r"_ZN3blz\d+k_mle_", n)]) == 12
