"""The on-device transcript (blz_ntt_fs_challenge) and the one-call prover (blz_ntt_sumcheck_prove), the part that needs no
device: both entry points exist in every layer with the signatures the header gives, a null handle is refused whatever else is
passed, the Python client's signatures, the host mirror of the transcript against hashlib with one fixed vector per field, the
transcript kernel lives in its own header and is compiled once, the prover reuses the step launchers behind the handle's slots,
the documents speak of both ops, and the shipped gfx950 code object holds what the kernel promises - ONE k_fs_ kernel, one
wave, no scratch, no LDS allocation, outside every existing kernel family, whose counts stay what they were."""
import ctypes
import hashlib
import inspect
import os
import random
import re

import pytest

import blaze_amd
from blaze_amd import fiat_shamir
from isa_util import ROOT, _read, count, disassemble_library, function_body, function_instructions, kernel_scratch, kernel_vgprs, tools_available
from oracle import pyref

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")
FS, PROVE = "blz_ntt_fs_challenge", "blz_ntt_sumcheck_prove"
FIELDS = ("BLS377", "BLS381", "BN254")
# the fragments the other ISA tests select their kernels by
FAMILIES = (r"k_gate_", r"k_vec_", r"k_sc_", r"k_mle_", r"k_fold_", r"k_horner_", r"k_gather_", r"k_spmv_", r"k_scatter_", r"k3", r"k_geval", r"k_lineval",
            r"k_zc_", r"k_tree_", r"k_ntt512_rr")


def test_declared_in_the_header_with_the_transcript_definition():
    hdr = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    arg = r"const\s+blz_vec_arg\s*\*\s*"
    assert re.search(rf"int\s+{FS}\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*void\s*\*\s*d_state\s*,\s*{arg}words\s*,\s*uint32_t\s+count\s*,\s*void\s*\*\s*d_r\s*\)\s*;", code)
    assert re.search(rf"int\s+{PROVE}\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*const\s+blz_sum_gate\s*\*\s*gate\s*,\s*{arg}tables\s*,\s*{arg}weight\s*,\s*uint32_t\s+points\s*,"
                     r"\s*uint64_t\s+len\s*,\s*void\s*\*\s*d_state\s*,\s*void\s*\*\s*d_rounds\s*,\s*void\s*\*\s*d_challenges\s*\)\s*;", code)
    # behind the types they take and the steps they chain
    assert code.index("} blz_sum_gate;") < code.index("blz_ntt_zerocheck_gate(") < code.index(FS + "(") < code.index(PROVE + "(")
    comment = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr[hdr.index("THE TRANSCRIPT STEP"):hdr.index(f"int {FS}(")]))
    for said in ("d_state is one 32-byte device word, 16-byte aligned. It is read and written.",
                 "digest = SHA3-256(state || w_0 || ... || w_{count-1}).",
                 "The w_i are the first `count` 32-byte words of `words`, exactly as stored. Nothing is reduced.",
                 "0 <= count <= 32. `words` may be NULL when count is 0.", "The new state is the digest.",
                 "with every bit from bit bitlen(modulus) - 1 upward cleared", "252 bits on BLS12-377, 254 on BLS12-381 and 253 on BN254",
                 "d_r is nullable; NULL means absorb only.", "d_state and d_r must not overlap each other or the words read.", "FIPS 202",
                 "BLZ_ERR_INVALID_PARAM"):
        assert said in comment, said
    comment = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", hdr[hdr.index("THE ONE-CALL PROVER"):hdr.index(f"int {PROVE}(")]))
    for said in ("weight == NULL", "the round alone at len writes d_rounds[0 .. points)", "absorbs row i of d_rounds", "len >> i", "the bind alone",
                 "top variable first", "at most len / 2 words of each table, at most len / 4 of the weight, and the three outputs",
                 "Everything is checked before the first launch", "NOT absorbed", "BLZ_ERR_INVALID_PARAM"):
        assert said in comment, said


def test_exported_and_bound():
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzSumGate, BlzVecArg
    P, V = ctypes.POINTER(BlzVecArg), ctypes.c_void_p
    assert EXPORTED_SYMBOLS.index(FS) == EXPORTED_SYMBOLS.index("blz_ntt_mle_tree") + 1 and EXPORTED_SYMBOLS.index(PROVE) == EXPORTED_SYMBOLS.index(FS) + 1
    assert _SIGS[FS] == (ctypes.c_int, [V, V, P, ctypes.c_uint32, V])
    assert _SIGS[PROVE] == (ctypes.c_int, [V, ctypes.POINTER(BlzSumGate), P, P, ctypes.c_uint32, ctypes.c_uint64, V, V, V])
    L = ctypes.CDLL(LIB)
    assert getattr(L, FS) is not None and getattr(L, PROVE) is not None
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.index("int blz_ntt_mle_tree(") < ntt.index(f"int {FS}(") < ntt.index(f"int {PROVE}(") < ntt.index("int blz_ntt_last_kernel_ms(")
    assert ntt.count(f"int {FS}(") == 1 and ntt.count(f"int {PROVE}(") == 1


def test_null_handle_is_refused_before_anything_else_is_looked_at():
    from blaze_amd._lib import BlzSumGate, BlzVecArg
    L = blaze_amd.lib()
    good, junk = BlzSumGate(1, 1, -1, 0), BlzSumGate(99, 0, -7, 5)
    good.term[0].nfactors = 1
    v, bad = BlzVecArg(None, 0, 0, 0), BlzVecArg(8, 7, 1, 3)
    r = ctypes.byref
    for args in ((None, None, 0, None), (16, r(v), 3, 32), (8, r(bad), 99, 8), (None, r(bad), 0xFFFFFFFF, None)):
        assert getattr(L, FS)(None, *args) == 4
        assert b"null handle" in L.blz_last_error_message()
    for args in ((r(good), r(v), None, 2, 4, 16, 32, 48), (r(junk), r(bad), r(bad), 77, 1 << 60, None, None, None), (None, None, None, 0, 3, 8, 8, 8),
                 (r(good), None, r(v), 0xFFFFFFFF, 0, None, 16, None)):
        assert getattr(L, PROVE)(None, *args) == 4
        assert b"null handle" in L.blz_last_error_message()


def test_python_client_signatures():
    from blaze_amd.ingo_ntt import NTTClient
    f = NTTClient.fs_challenge
    assert list(inspect.signature(f).parameters) == ["self", "state", "words", "count", "r"]
    assert f.__defaults__ == (None, None, None)   # the state is required
    assert "_vec_keep" in f.__code__.co_names and FS in f.__code__.co_names
    g = NTTClient.sumcheck_prove
    assert list(inspect.signature(g).parameters) == ["self", "tables", "terms", "state", "weight", "common", "points", "length", "rounds", "challenges"]
    assert g.__defaults__ == (None, None, None, None, None, None)
    assert "_vec_keep" in g.__code__.co_names and PROVE in g.__code__.co_names and "_sum_gate" in g.__code__.co_names
    assert "fiat_shamir" in f.__doc__ and "fiat_shamir" in g.__doc__


# SHA3-256(32 zero bytes || 2 || 3 as 256-bit little-endian words): a digest with its top four bits set, so that the three
# fields' masks give three different challenges
KNOWN_STATE = bytes.fromhex("90563e549b608dfc18616113e304cdaa334a045bacc2e218580bc6f15f41d6f2")
KNOWN_CHALLENGE = {"BLS377": 0x2d6415ff1c60b5818e2c2ac5b044a33aacd04e313616118fc8d609b543e5690,
                   "BLS381": 0x32d6415ff1c60b5818e2c2ac5b044a33aacd04e313616118fc8d609b543e5690,
                   "BN254": 0x12d6415ff1c60b5818e2c2ac5b044a33aacd04e313616118fc8d609b543e5690}


def test_host_mirror_against_hashlib():
    assert hashlib.sha3_256(b"").hexdigest() == "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a"   # FIPS 202's own vector
    assert [fiat_shamir.challenge_bits(f) for f in FIELDS] == [252, 254, 253]
    rng = random.Random(5)
    for field in FIELDS:
        r = pyref.CURVES[field]["r"]
        assert fiat_shamir.MODULUS[field] == r and fiat_shamir.challenge_bits(field) == r.bit_length() - 1
        assert fiat_shamir.absorb(bytes(32), [2, 3], field) == (KNOWN_STATE, KNOWN_CHALLENGE[field])
        assert KNOWN_CHALLENGE[field] == int.from_bytes(KNOWN_STATE, "little") % (1 << (r.bit_length() - 1)) < r
        # 3 | 4 words: 128 | 160 bytes, on either side of the 136-byte rate; 16: 544 = 4 x 136, the padding a block of its own
        for count in (0, 1, 3, 4, 16, 17, 32):
            state = rng.randbytes(32)
            words = [0, r - 1, r, (1 << 256) - 1][:count] + [rng.getrandbits(256) for _ in range(max(count - 4, 0))]
            raw = b"".join(w.to_bytes(32, "little") for w in words)
            assert len(state + raw) == 32 * (1 + count)
            digest = hashlib.sha3_256(state + raw).digest()
            want = (digest, int.from_bytes(digest, "little") & ((1 << (r.bit_length() - 1)) - 1))
            assert fiat_shamir.absorb(state, words, field) == want   # ints
            assert fiat_shamir.absorb(state, raw, field) == want     # the bytes as downloaded
            assert fiat_shamir.absorb(state, [raw[i:i + 32] for i in range(0, len(raw), 32)], field) == want
            assert want[1] < 1 << (r.bit_length() - 1)
        # a chain: each row's state is the next one's
        rows = [rng.randbytes(96) for _ in range(5)]
        state, chal = fiat_shamir.challenges(bytes(32), rows, field)
        s = bytes(32)
        for row, x in zip(rows, chal):
            s, y = fiat_shamir.absorb(s, row, field)
            assert x == y
        assert s == state
    for bad in (lambda: fiat_shamir.absorb(bytes(31), []), lambda: fiat_shamir.absorb(bytes(32), bytes(33)), lambda: fiat_shamir.absorb(bytes(32), [0] * 33),
                lambda: fiat_shamir.absorb(bytes(32), [1 << 256])):
        with pytest.raises((ValueError, OverflowError)):
            bad()


def test_mirrors():
    hpp = _read("include", "blaze.hpp")
    assert re.search(r"void\s+fs_challenge\s*\(\s*void\s*\*\s*d_state\s*,", hpp) and FS + "(" in hpp
    assert re.search(r"void\s+sumcheck_prove\s*\(\s*const\s+blz_sum_gate\s*&", hpp) and PROVE + "(" in hpp
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_fs_challenge\(h: \*mut BlzNtt, d_state: \*mut c_void, words: \*const BlzVecArg, count: u32, d_r: \*mut c_void\) -> c_int;", ffi)
    assert re.search(r"pub fn blz_ntt_sumcheck_prove\(h: \*mut BlzNtt, gate: \*const BlzSumGate, tables: \*const BlzVecArg, weight: \*const BlzVecArg, points: u32,"
                     r"\s*len: u64, d_state: \*mut c_void, d_rounds: \*mut c_void, d_challenges: \*mut c_void\) -> c_int;", ffi)
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "pub unsafe fn fs_challenge(" in api and FS + "(" in api and "pub unsafe fn sumcheck_prove(" in api and PROVE + "(" in api


def test_kernel_in_its_own_header_compiled_once():
    src = _read("blaze_amd", "csrc", "ntt_fs.hip.hpp")
    assert re.findall(r"__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", src) == ["k_fs_absorb"] and "template" not in src   # field-independent
    statements = re.sub(r"//[^\n]*", "", src)
    for banned in ("atomic", "alloc", "volatile", "__threadfence", "__shared__", "__syncthreads", "asm"):
        assert banned not in statements, banned
    assert "__launch_bounds__(64)" in statements and "dim3(1), dim3(64)" in statements   # one wave
    # cross-lane reads, and not one lane running the rounds by itself
    assert statements.count("__shfl(") == 9
    # compiled with ntt.hip alone: the per-field sources do not see it
    assert '#include "ntt_fs.hip.hpp"' in _read("blaze_amd", "csrc", "ntt.hip")
    for other in ("ntt_impl.hip.hpp", "ntt_engine.hpp", "ntt_bls381.hip", "ntt_bls377.hip", "ntt_bn254.hip"):
        assert "ntt_fs" not in _read("blaze_amd", "csrc", other), other


def test_entry_points_check_first_and_reuse_the_steps():
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    body = function_body(ntt, f"int {PROVE}(")
    # the step launchers behind the handle's slots, the shared description check, ONE enqueue for the whole chain
    for once in ("h->ops->sumcheck_gate(", "h->ops->zerocheck_gate(", "ntt_prove_describe(", "call.begin()", "call.live_length(", "call.resolve(", "call.enqueue("):
        assert body.count(once) == 1, once
    assert ntt.count("ntt_prove_describe = &ntt_gate_describe;") == 1 and '"gate: ' not in body
    assert body.index('"null handle"') < body.index("ntt_prove_describe(") < body.index("call.live_length(") < body.index("call.begin()") \
        < body.index("call.resolve(") < body.index("call.device_range(") < body.index("call.enqueue(")
    for waits in ("hipStreamSynchronize", "sync_stream_bounded", "hipMemcpy", "hipEventSynchronize", "hipLaunchKernelGGL"):
        assert waits not in body, waits
    assert body.count("ntt_fs_absorb(") == 1 and body[body.index("call.enqueue("):].count("step(") == 3
    fs = function_body(ntt, f"int {FS}(")
    for once in ("call.begin()", "call.resolve(", "call.enqueue(", "ntt_fs_absorb("):
        assert fs.count(once) == 1, once
    assert fs.index('"null handle"') < fs.index("null d_state") < fs.index("FS_MAX_WORDS") < fs.index("call.begin()") < fs.index("call.resolve(") < fs.index("call.enqueue(")
    # the step ops and their protocol are as they were
    shared = function_body(ntt, "int ntt_step_protocol(")
    assert shared.count("NttVecCall::words_meet(") == 3 and "ntt_fs" not in shared


def test_documented_where_the_other_ops_are():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md"):
        text = _read(doc)
        assert "fs_challenge" in text and "sumcheck_prove" in text, doc
    design = _read("DESIGN.md")
    assert "**One-call prover**" in design and "k_fs_absorb" in design and "SHA3-256" in design
    assert "ntt_prove_timing.py" in design and "ntt_prove.json" in design
    section = design[design.index("**One-call prover**"):]
    for kept_out in ("Out of scope", "algebraic transcript", "final table words", "GKR", "1024"):
        assert kept_out in section, kept_out
    assert os.path.exists(os.path.join(ROOT, "tools", "ntt_prove_timing.py"))
    assert os.path.exists(os.path.join(ROOT, "blaze_amd", "fiat_shamir.py"))


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    return kernel_vgprs(LIB), kernel_scratch(LIB), disassemble_library(LIB)


def test_one_transcript_kernel_without_scratch_outside_the_families(code):
    vgprs, scratch, text = code
    names = sorted(n for n in vgprs if "k_fs_" in n)
    print({n: (vgprs[n], scratch[n]) for n in names})
    assert names == ["_ZN3blz11k_fs_absorbEPmPKmjS0_j"], names   # one copy: no field in its name
    n = names[0]
    assert scratch[n] == 0 and vgprs[n] <= 64, (vgprs[n], scratch[n])
    for family in FAMILIES:
        assert not re.match(rf"_ZN3blz\d+{family}", n), family
    assert "poseidon" not in n and "Fr_" not in n
    ins = function_instructions(text, n)
    # nine 64-bit cross-lane reads a round, two ds_bpermute_b32 each, in a loop that is not unrolled; no field arithmetic
    assert 18 <= count(ins, "ds_bpermute_b32") <= 40, count(ins, "ds_bpermute_b32")
    assert count(ins, "v_mad_u64_u32") < 16   # (addresses; a Montgomery product is 128 of them)
    # the neighbours keep their counts
    for family, kept in ((r"k_gate_", 6), (r"k_sc_", 33), (r"k_zc_", 6), (r"k_mle_", 12), (r"k_tree_", 24)):
        assert len([k for k in vgprs if re.match(rf"_ZN3blz\d+{family}", k)]) == kept, family
