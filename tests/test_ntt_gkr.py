"""The one-call GKR grand-product prover (blz_ntt_gkr_prove), the part that needs no device: the entry point exists in every
layer with the signature the header gives and behind blz_ntt_sumcheck_prove, a null handle is refused whatever else is passed,
the Python client's signature, the layout arithmetic, the verifier (blaze_amd/gkr.py) against a prover written here on Python
integers - accepted, and rejected with the layer named when one word is flipped -, the kernels live in their own header behind one
NttFieldOps slot, the entry point's checks stand in the documented order, the documents speak of the op, and the shipped gfx950
code object holds what the kernel promises - three k_gkr_tail and three k_gkr_claims, no scratch, VGPRs under the next occupancy
step, static LDS within 64 KiB - with every other family's count unchanged."""
import ctypes
import inspect
import os
import random
import re

import pytest

import blaze_amd
from blaze_amd import fiat_shamir, gkr
from isa_util import ROOT, _read, count, disassemble_library, function_body, function_instructions, kernel_scratch, kernel_vgprs, tools_available
from ntt_gkr_util import mle_at, prove_ref

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("BLS381", "BLS377", "BN254")
MANGLED = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
NAME, PROVE = "blz_ntt_gkr_prove", "blz_ntt_sumcheck_prove"


def _uncommented(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_declared_in_the_header_behind_the_one_call_prover():
    raw = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    arg, ptr = r"const\s+blz_vec_arg\s*\*\s*", r"void\s*\*\s*"
    assert re.search(rf"int\s+{NAME}\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*uint32_t\s+op\s*,\s*uint32_t\s+flags\s*,\s*{arg}tree\s*,\s*{arg}a\s*,\s*uint64_t\s+len\s*,"
                     rf"\s*{ptr}d_weight\s*,\s*{ptr}d_state\s*,\s*{ptr}d_rounds\s*,\s*{ptr}d_points\s*,\s*{ptr}d_claims\s*\)\s*;", code)
    assert re.search(r"#define\s+BLZ_GKR_UNFUSED\s+1u?\b", code)
    assert code.index(PROVE + "(") < code.index(NAME + "(") < code.index("blz_device_malloc(")
    assert not re.search(r"\bblz_[a-z0-9_]+\s*\(", code[code.index(PROVE + "(") + len(PROVE) + 1: code.index(NAME + "(")])
    # the comment block: its heading, the layout of section 1, the bytes written, the order of checks
    assert raw.index(f"int {PROVE}(") < raw.index("THE ONE-CALL GKR PROVER") < raw.index(f"int {NAME}(")
    comment = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", raw[raw.index("THE ONE-CALL GKR PROVER"):raw.index(f"int {NAME}(")]))
    for said in ("3 m (m - 1) / 2 words", "m (m + 1) / 2 words", "2 m words", "3 (j (j - 1) / 2 + i)", "word j - 1 - i of row j", "BYTES WRITTEN",
                 "The root is NOT absorbed", "BLZ_TREE_FRAC is refused by name", "in this order: a null handle", "BLZ_GKR_UNFUSED", "verify_product"):
        assert said in comment, said


def test_defined_between_the_one_call_prover_and_last_kernel_ms():
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.index(f"int {PROVE}(") < ntt.index(f"int {NAME}(") < ntt.index("int blz_ntt_last_kernel_ms(")
    assert ntt.count(f"int {NAME}(") == 1


def test_exported_and_bound():
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzVecArg
    assert EXPORTED_SYMBOLS.index(NAME) == EXPORTED_SYMBOLS.index(PROVE) + 1
    P, V = ctypes.POINTER(BlzVecArg), ctypes.c_void_p
    assert _SIGS[NAME] == (ctypes.c_int, [V, ctypes.c_uint32, ctypes.c_uint32, P, P, ctypes.c_uint64, V, V, V, V, V])
    assert getattr(ctypes.CDLL(LIB), NAME) is not None


def test_null_handle_is_refused_before_anything_else_is_looked_at():
    from blaze_amd._lib import BlzVecArg
    L = blaze_amd.lib()
    v, bad = BlzVecArg(None, 0, 0, 0), BlzVecArg(8, 7, 1, 3)
    r = ctypes.byref
    for args in ((0, 0, r(v), r(v), 4, 16, 16, 16, 16, 16), (1, 1, r(bad), r(bad), 8, None, None, None, None, None), (99, 0xFFFFFFFF, None, None, 0, 1, 2, 3, 4, 5),
                 (0, 2, r(v), None, 1 << 60, None, 8, None, 8, None), (0, 0, None, r(bad), 0xFFFFFFFFFFFFFFFF, 7, 7, 7, 7, 7)):
        assert getattr(L, NAME)(None, *args) == 4
        assert b"null handle" in L.blz_last_error_message()


def test_python_signatures():
    from blaze_amd.ingo_ntt import NTTClient
    assert NTTClient.GKR_UNFUSED == 1
    f = NTTClient.gkr_prove
    assert callable(f) and "_vec_keep" in f.__code__.co_names and NAME in f.__code__.co_names
    sig = inspect.signature(f)
    assert list(sig.parameters) == ["self", "tree", "a", "state", "length", "weight", "rounds", "points", "claims", "fused"]
    assert [sig.parameters[p].default for p in ("length", "weight", "rounds", "points", "claims", "fused")] == [None] * 5 + [True]
    assert all(sig.parameters[p].default is inspect.Parameter.empty for p in ("tree", "a", "state"))
    assert "gkr.verify_product" in f.__doc__
    assert gkr.TAIL_LEN == 512
    assert list(inspect.signature(gkr.layout).parameters) == ["m"]
    assert list(inspect.signature(gkr.verify_product).parameters) == ["field", "m", "root", "state", "rounds", "points", "claims"]


def test_mirrors():
    hpp = _read("include", "blaze.hpp")
    assert NAME + "(" in hpp and re.search(r"void\s+gkr_prove\s*\(\s*const\s+blz_vec_arg\s*\*\s*tree\s*,", hpp) and "BLZ_GKR_UNFUSED" in hpp
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_gkr_prove\(h: \*mut BlzNtt, op: u32, flags: u32, tree: \*const BlzVecArg, a: \*const BlzVecArg, len: u64, d_weight: \*mut c_void,"
                     r"\s*d_state: \*mut c_void, d_rounds: \*mut c_void, d_points: \*mut c_void, d_claims: \*mut c_void\) -> c_int;", ffi)
    assert "pub const BLZ_GKR_UNFUSED: u32 = 1;" in ffi
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "pub unsafe fn gkr_prove(" in api and NAME + "(" in api and "pub fn gkr_layout(" in api


def test_layout_against_the_formulas():
    for m in range(1, 28):
        lay = gkr.layout(m)
        assert (lay.m, lay.rounds_words, lay.points_words, lay.claims_words) == (m, 3 * m * (m - 1) // 2, m * (m + 1) // 2, 2 * m)
        assert lay.weight_words == max((1 << m) // 4, 1)
        assert len(lay.rounds) == len(lay.points) == len(lay.claims) == m
        for j in range(m):
            assert lay.rounds[j] == 3 * (j * (j - 1) // 2) and lay.points[j] == j * (j + 1) // 2 and lay.claims[j] == 2 * j
        # rows back to back: layer j has j rounds of three words, j + 1 point words and two claims
        assert all(lay.rounds[j] + 3 * j == lay.rounds[j + 1] for j in range(m - 1)) and lay.rounds[m - 1] + 3 * (m - 1) == lay.rounds_words
        assert all(lay.points[j] + j + 1 == lay.points[j + 1] for j in range(m - 1)) and lay.points[m - 1] + m == lay.points_words
    for m in (0, -1):
        with pytest.raises(ValueError):
            gkr.layout(m)


_PROOFS = {}


def _proof(field, m):
    """A proof by the Python prover over random words (more than half of them above the modulus), computed once"""
    if (field, m) not in _PROOFS:
        rng = random.Random(4100 + 10 * m + len(field))
        leaves = [int.from_bytes(rng.randbytes(32), "little") for _ in range(1 << m)]
        state0 = rng.randbytes(32)
        _PROOFS[field, m] = (leaves, state0) + prove_ref(field, leaves, state0)
    return _PROOFS[field, m]


def _pack(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m", (1, 2, 5))
def test_verifier_accepts_the_python_prover(field, m):
    r = fiat_shamir.MODULUS[field]
    leaves, state0, root, rounds, points, claims, final = _proof(field, m)
    lay = gkr.layout(m)
    assert (len(rounds), len(points), len(claims)) == (lay.rounds_words, lay.points_words, lay.claims_words)
    prod = 1
    for v in leaves:
        prod = prod * v % r
    assert root == prod
    for as_bytes in (False, True):
        args = [_pack(x) if as_bytes else x for x in (rounds, points, claims)]
        state, point, claim = gkr.verify_product(field, m, root, state0, *args)
        assert state == final and point == points[lay.points[m - 1]:] and len(point) == m
        # the leaves' claim is their multilinear extension at the point: sum_p eq(point, p) leaf[p]
        assert claim == mle_at(leaves, point, r)
        want = 0
        for p, v in enumerate(leaves):
            e = 1
            for i, t in enumerate(point):
                e = e * (t if (p >> i) & 1 else 1 - t) % r
            want += e * v
        assert claim == want % r


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m", (1, 2, 5))
def test_verifier_rejects_one_flipped_word_and_names_the_layer(field, m):
    leaves, state0, root, rounds, points, claims, _ = _proof(field, m)
    lay = gkr.layout(m)

    def refused(match, root=root, rounds=rounds, points=points, claims=claims):
        with pytest.raises(ValueError, match=match):
            gkr.verify_product(field, m, root, state0, rounds, points, claims)

    def flipped(words, at):
        return words[:at] + [words[at] ^ 1] + words[at + 1:]

    refused(r"layer 0\b", root=root ^ 1)
    for j in range(m):
        for t in range(2):   # each claim word: the layer's final check
            refused(rf"layer {j}\b", claims=flipped(claims, lay.claims[j] + t))
        refused(rf"layer {j}\b", points=flipped(points, lay.points[j] + j))   # rho_j
        for i in range(j):
            for t in range(3):   # u_i(0) and u_i(1) fail the sum, u_i(2) the challenge derived from the row
                refused(rf"layer {j}, round {i}\b", rounds=flipped(rounds, lay.rounds[j] + 3 * i + t))
            refused(rf"layer {j}, round {i}\b", points=flipped(points, lay.points[j] + j - 1 - i))
    # a proof that is consistent with itself, but from another transcript state
    with pytest.raises(ValueError, match=r"layer 0\b"):   # the first challenge, rho_0, is not that state's
        gkr.verify_product(field, m, root, bytes(32), rounds, points, claims)


def test_kernels_in_their_own_header_behind_one_slot():
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    eng = _read("blaze_amd", "csrc", "ntt_engine.hpp")
    assert impl.index('#include "ntt_tree.hip.hpp"') < impl.index('#include "ntt_gkr.hip.hpp"')
    assert impl.count("o.gkr_tail = ") == 1 and len(re.findall(r"\(\*gkr_tail\)\s*\(\s*hipStream_t\s+st\s*,", eng)) == 1
    assert re.search(r"constexpr\s+uint32_t\s+GKR_TAIL_LEN\s*=\s*1u\s*<<\s*GKR_TAIL_LOG\s*;", eng) and re.search(r"constexpr\s+int\s+GKR_TAIL_LOG\s*=\s*9\s*;", eng)
    src = _read("blaze_amd", "csrc", "ntt_gkr.hip.hpp")
    kernels = re.findall(r"template\s*<([^>]*)>\s*__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", src)
    assert kernels == [("class Fr", "k_gkr_tail"), ("class Fr", "k_gkr_claims")], kernels
    statements = _uncommented(src)
    for banned in ("atomic", "alloc", "volatile", "__threadfence", "asm", "ws", "while (true)", "for (;;)"):
        assert not re.search(rf"\b{re.escape(banned)}", statements), banned
    # the transcript's header is not visible to the per-field sources: the permutation here is this header's own
    assert "ntt_fs" not in statements and "FS_ROUND_CONSTANTS" not in statements and "GKR_KECCAK_RC[24]" in statements
    # every lane of the one block reaches every barrier: nothing returns out of the kernels, and wave 0's transcript holds none
    body = statements[statements.index("void k_gkr_tail("): statements.index("void k_gkr_claims(")]
    assert "return" not in body and body.count("__syncthreads()") >= 6
    lines = body.split("\n")
    heads = [k for k, ln in enumerate(lines) if ln.strip() == "if (wave0) {"]
    assert len(heads) == 2 and body.count("wave0)") == 2
    for k in heads:
        indent = lines[k][:len(lines[k]) - len(lines[k].lstrip())]
        end = next(e for e in range(k + 1, len(lines)) if lines[e] == indent + "}")
        assert "__syncthreads" not in "\n".join(lines[k:end]) and "gkr_absorb(" in "\n".join(lines[k:end])
    # the state is read once and stored once; no table word, no weight word goes back to memory
    assert body.count("g.state") == 2 and not re.search(r"fp_store\(\s*(gl|gh|g\.tree|g\.a|g\.weight)\b", body)
    # the existing launchers and the transcript header are as they were
    assert re.findall(r"__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", _read("blaze_amd", "csrc", "ntt_fs.hip.hpp")) == ["k_fs_absorb"]
    assert "k_gkr_" not in _read("blaze_amd", "csrc", "ntt.hip").replace("k_gkr_claims, a copy of two words", "")


def test_entry_point_checks_first_in_the_documented_order():
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    body = function_body(ntt, f"int {NAME}(")
    for once in ("call.begin()", "call.live_length(", "call.resolve(", "call.enqueue(", "call.device_range(", "NttVecCall::words_meet(", "h->ops->vec_mle_eq(",
                 "h->ops->sumcheck_gate("):
        assert body.count(once) == 1, once
    assert body.count("h->ops->zerocheck_gate(") == 2 and body.count("ntt_fs_absorb(") == 2 and body.count("h->ops->gkr_tail(") == 3
    order = ['"null handle"', "BLZ_TREE_FRAC is not built", "unknown tree op", "unknown GKR flags", "tree is NULL", "a is NULL", "d_weight is NULL",
             "d_state is NULL", "d_rounds is NULL", "d_points is NULL", "d_claims is NULL", "call.live_length(", "call.begin()", "call.resolve(",
             "call.device_range(", "NttVecCall::words_meet(", "call.enqueue("]
    at = [body.index(s) for s in order]
    assert at == sorted(at), list(zip(order, at))
    # nothing is launched ahead of the enqueue, and nothing waits for the device or copies through the host
    head = body[:body.index("call.enqueue(")]
    for launched in ("h->ops->", "ntt_fs_absorb(", "hipLaunchKernelGGL"):
        assert launched not in head, launched
    for waits in ("hipStreamSynchronize", "sync_stream_bounded", "hipMemcpy", "hipEventSynchronize", "hipLaunchKernelGGL"):
        assert waits not in body, waits
    # the one-call prover itself is as it was
    prove = function_body(ntt, f"int {PROVE}(")
    assert "gkr" not in prove and prove.count("ntt_fs_absorb(") == 1


def test_documented_where_the_other_ops_are():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md"):
        assert "gkr_prove" in _read(doc), doc
    design = _read("DESIGN.md")
    assert "**One-call GKR**" in design and design.index("**One-call prover**") < design.index("**One-call GKR**")
    section = design[design.index("**One-call GKR**"):]
    for said in ("k_gkr_tail", "GKR_TAIL_LEN", "512", "80 KiB", "VGPR", "ntt_gkr_timing.py", "ntt_gkr.json", "Out of scope", "BLZ_TREE_FRAC"):
        assert said in section, said
    assert os.path.exists(os.path.join(ROOT, "tools", "ntt_gkr_timing.py"))


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    notes = disassemble_library(LIB, "llvm-readelf", "--notes")
    # (a kernel's map is sorted by key: .group_segment_fixed_size comes before .name)
    lds = {n: int(v) for v, n in re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\s+\.group_segment_fixed_size:).*\n)*?\s+\.name:\s+(\S+)", notes)}
    return kernel_vgprs(LIB), kernel_scratch(LIB), lds, disassemble_library(LIB)


VGPR_CAP = 128   # the next occupancy step above the 123 - 126 the compiler reports: four waves per SIMD ("One-call GKR")
LDS_CAP = 64 * 1024   # what a static allocation may have


def test_three_tails_and_three_claims_without_scratch_within_the_caps(code):
    vgprs, scratch, lds, text = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_gkr_", n))
    print({n: (vgprs[n], scratch[n], lds[n]) for n in names})
    assert names == sorted(f"_ZN3blz{k}INS_{f}EEEvNS_10NttGkrTailE" for k in ("10k_gkr_tail", "12k_gkr_claims") for f in MANGLED), names
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= VGPR_CAP, (n, vgprs[n])
        assert lds[n] <= LDS_CAP, (n, lds[n])
        assert "poseidon" not in n
        ins = function_instructions(text, n)
        if "k_gkr_tail" in n:
            # two tables of 512 words and a weight of 256 are 40 KiB; the field products are inlined; the permutation runs on
            # cross-lane reads; the block meets at barriers
            assert lds[n] >= 40 * 1024, lds[n]
            assert count(ins, "v_mad_u64_u32") >= 256, n
            assert count(ins, "ds_bpermute_b32") >= 18 and count(ins, "s_barrier") >= 6, n
        else:
            assert lds[n] == 0 and vgprs[n] <= 16 and count(ins, "v_mad_u64_u32") < 16, n
    # the neighbours keep their counts
    for family, kept in ((r"k_gate_", 6), (r"k_sc_", 33), (r"k_zc_", 6), (r"k_mle_", 12), (r"k_tree_", 24), (r"k_fs_", 1)):
        assert len([k for k in vgprs if re.match(rf"_ZN3blz\d+{family}", k)]) == kept, family
