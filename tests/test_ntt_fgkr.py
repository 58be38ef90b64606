"""The one-call fraction GKR prover (blz_ntt_gkr_prove_frac, logUp-GKR), the part that needs no device: the entry point exists in
every layer with the signature the header gives and directly behind blz_ntt_gkr_prove, a null handle is refused whatever else is
passed, the Python client's signature, the layout arithmetic, the verifier (blaze_amd/gkr.py verify_fraction) against a prover
written on Python integers (ntt_fgkr_util) - accepted, and rejected with the layer named when one word is flipped -, a logUp
instance whose root numerator is 0 exactly when every lookup is in the table, the kernels live in their own header behind one
NttFieldOps slot, the entry point's checks stand in the documented order, the documents speak of the op, and the shipped gfx950
code object holds what the kernel promises - three k_fgkr_tail and three k_fgkr_claims, no scratch, VGPRs under the next
occupancy step, static LDS between 36 and 64 KiB."""
import ctypes
import inspect
import os
import random
import re

import pytest

import blaze_amd
from blaze_amd import fiat_shamir, gkr
from isa_util import ROOT, _read, count, disassemble_library, function_body, function_instructions, kernel_scratch, kernel_vgprs, tools_available
from ntt_fgkr_util import frac_trees, logup_instance, prove_ref
from ntt_gkr_util import mle_at

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

FIELDS = ("BLS381", "BLS377", "BN254")
MANGLED = ("9Fr_BLS381", "9Fr_BLS377", "8Fr_BN254")
NAME, GKR, PROVE = "blz_ntt_gkr_prove_frac", "blz_ntt_gkr_prove", "blz_ntt_sumcheck_prove"
HEADING = "THE ONE-CALL FRACTION GKR PROVER"


def _uncommented(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_declared_in_the_header_directly_behind_the_grand_product():
    raw = _read("include", "blaze_hip.h")
    code = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    arg, ptr = r"const\s+blz_vec_arg\s*\*\s*", r"void\s*\*\s*"
    assert re.search(rf"int\s+{NAME}\s*\(\s*blz_ntt\s*\*\s*h\s*,\s*uint32_t\s+flags\s*,\s*{arg}tree_p\s*,\s*{arg}tree_q\s*,\s*{arg}a_p\s*,\s*{arg}a_q\s*,"
                     rf"\s*uint64_t\s+len\s*,\s*{ptr}d_weight\s*,\s*{ptr}d_state\s*,\s*{ptr}d_rounds\s*,\s*{ptr}d_points\s*,\s*{ptr}d_claims\s*,"
                     rf"\s*{ptr}d_lambdas\s*\)\s*;", code)
    assert code.index(PROVE + "(") < code.index(GKR + "(") < code.index(NAME + "(") < code.index("blz_device_malloc(")
    # nothing between the one-call prover and the grand product, nothing between the grand product and this
    for a, b in ((PROVE, GKR), (GKR, NAME)):
        assert not re.search(r"\bblz_[a-z0-9_]+\s*\(", code[code.index(a + "(") + len(a) + 1: code.index(b + "(")]), (a, b)
    assert raw.index(f"int {GKR}(") < raw.index(HEADING) < raw.index(f"int {NAME}(")
    comment = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", raw[raw.index(HEADING):raw.index(f"int {NAME}(")]))
    for said in ("3 m (m - 1) / 2 words", "m (m + 1) / 2 words", "4 m words", "m words", "3 (j (j - 1) / 2 + i)", "word j - 1 - i of row j", "BYTES WRITTEN",
                 "The roots are NOT absorbed", "in this order: a null handle", "BLZ_GKR_UNFUSED", "verify_fraction", "T = P_hi + lambda_j Q_hi",
                 "Word 0 is never written", "count 0", "two blocks", "T_f - lambda_j Q_hi_f", "d_weight, d_state, d_rounds, d_points, d_claims, d_lambdas"):
        assert said in comment, said
    # the grand product still refuses fraction trees, by name
    assert "BLZ_TREE_FRAC is refused by name" in raw and "BLZ_TREE_FRAC is not built" in _read("blaze_amd", "csrc", "ntt.hip")


def test_defined_between_the_grand_product_and_last_kernel_ms():
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert ntt.index(f"int {GKR}(") < ntt.index(f"int {NAME}(") < ntt.index("int blz_ntt_last_kernel_ms(")
    assert ntt.count(f"int {NAME}(") == 1 and ntt.count(f"int {GKR}(") == 1


def test_exported_and_bound():
    from blaze_amd._lib import _SIGS, EXPORTED_SYMBOLS, BlzVecArg
    assert EXPORTED_SYMBOLS.index(NAME) == EXPORTED_SYMBOLS.index(GKR) + 1
    P, V = ctypes.POINTER(BlzVecArg), ctypes.c_void_p
    assert _SIGS[NAME] == (ctypes.c_int, [V, ctypes.c_uint32, P, P, P, P, ctypes.c_uint64, V, V, V, V, V, V])
    assert getattr(ctypes.CDLL(LIB), NAME) is not None


def test_null_handle_is_refused_before_anything_else_is_looked_at():
    from blaze_amd._lib import BlzVecArg
    L = blaze_amd.lib()
    v, bad = BlzVecArg(None, 0, 0, 0), BlzVecArg(8, 7, 1, 3)
    r = ctypes.byref
    for args in ((0, r(v), r(v), r(v), r(v), 4, 16, 16, 16, 16, 16, 16), (1, r(bad), r(bad), r(bad), r(bad), 8, None, None, None, None, None, None),
                 (0xFFFFFFFF, None, None, None, None, 0, 1, 2, 3, 4, 5, 6), (2, r(v), None, r(v), None, 1 << 60, None, 8, None, 8, None, 8),
                 (0, None, r(bad), None, r(bad), 0xFFFFFFFFFFFFFFFF, 7, 7, 7, 7, 7, 7)):
        assert getattr(L, NAME)(None, *args) == 4
        assert b"null handle" in L.blz_last_error_message()


def test_python_signatures():
    from blaze_amd.ingo_ntt import NTTClient
    f = NTTClient.gkr_prove_frac
    assert callable(f) and "_vec_keep" in f.__code__.co_names and NAME in f.__code__.co_names
    sig = inspect.signature(f)
    assert list(sig.parameters) == ["self", "tree_p", "tree_q", "a_p", "a_q", "state", "length", "weight", "rounds", "points", "claims", "lambdas", "fused"]
    assert [sig.parameters[p].default for p in ("length", "weight", "rounds", "points", "claims", "lambdas", "fused")] == [None] * 6 + [True]
    assert all(sig.parameters[p].default is inspect.Parameter.empty for p in ("tree_p", "tree_q", "a_p", "a_q", "state"))
    assert "gkr.verify_fraction" in f.__doc__ and "gkr.layout_frac" in f.__doc__
    assert list(inspect.signature(gkr.layout_frac).parameters) == ["m"]
    assert list(inspect.signature(gkr.verify_fraction).parameters) == ["field", "m", "root_p", "root_q", "state", "rounds", "points", "claims", "lambdas"]
    # the grand product's mirrors are as they were
    assert list(inspect.signature(gkr.layout).parameters) == ["m"] and gkr.layout(3).claims_words == 6
    assert list(inspect.signature(gkr.verify_product).parameters) == ["field", "m", "root", "state", "rounds", "points", "claims"]


def test_mirrors():
    hpp = _read("include", "blaze.hpp")
    assert NAME + "(" in hpp and re.search(r"void\s+gkr_prove_frac\s*\(\s*const\s+blz_vec_arg\s*\*\s*tree_p\s*,", hpp)
    ffi = _read("rust", "src", "driver_client", "hip_ffi.rs")
    assert re.search(r"pub fn blz_ntt_gkr_prove_frac\(h: \*mut BlzNtt, flags: u32, tree_p: \*const BlzVecArg, tree_q: \*const BlzVecArg, a_p: \*const BlzVecArg,"
                     r"\s*a_q: \*const BlzVecArg, len: u64, d_weight: \*mut c_void, d_state: \*mut c_void, d_rounds: \*mut c_void, d_points: \*mut c_void,"
                     r"\s*d_claims: \*mut c_void, d_lambdas: \*mut c_void\) -> c_int;", ffi)
    api = _read("rust", "src", "ingo_ntt", "ntt_api.rs")
    assert "pub unsafe fn gkr_prove_frac(" in api and NAME + "(" in api and "pub fn gkr_layout_frac(" in api


def test_layout_against_the_formulas():
    for m in range(1, 28):
        lay, prod = gkr.layout_frac(m), gkr.layout(m)
        assert (lay.m, lay.rounds_words, lay.points_words, lay.claims_words, lay.lambdas_words) == (m, 3 * m * (m - 1) // 2, m * (m + 1) // 2, 4 * m, m)
        assert lay.weight_words == max((1 << m) // 4, 1)
        assert len(lay.rounds) == len(lay.points) == len(lay.claims) == m
        for j in range(m):
            assert lay.rounds[j] == 3 * (j * (j - 1) // 2) and lay.points[j] == j * (j + 1) // 2 and lay.claims[j] == 4 * j
        assert (lay.rounds, lay.points, lay.rounds_words, lay.points_words) == (prod.rounds, prod.points, prod.rounds_words, prod.points_words)
    for m in (0, -1):
        with pytest.raises(ValueError):
            gkr.layout_frac(m)


_PROOFS = {}


def _proof(field, m):
    """A proof by the Python prover over random words (more than half of them above the modulus), computed once:
    (a_p, a_q, state0, root_p, root_q, rounds, points, claims, lambdas, final state), lambdas[0] set to a marker"""
    if (field, m) not in _PROOFS:
        r = fiat_shamir.MODULUS[field]
        rng = random.Random(4700 + 10 * m + len(field))
        while True:   # BLS12-381's modulus is 0.45 x 2^256: a draw of few words may miss the majority
            a_p, a_q = ([int.from_bytes(rng.randbytes(32), "little") for _ in range(1 << m)] for _ in range(2))
            if sum(v >= r for v in a_p) > len(a_p) // 2 and sum(v >= r for v in a_q) > len(a_q) // 2:
                break
        state0 = rng.randbytes(32)
        root_p, root_q, rounds, points, claims, lambdas, final = prove_ref(field, a_p, a_q, state0)
        _PROOFS[field, m] = (a_p, a_q, state0, root_p, root_q, rounds, points, claims, [0xABCD] + lambdas[1:], final)
    return _PROOFS[field, m]


def _pack(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m", (1, 2, 5))
def test_verifier_accepts_the_python_prover(field, m):
    r = fiat_shamir.MODULUS[field]
    a_p, a_q, state0, root_p, root_q, rounds, points, claims, lambdas, final = _proof(field, m)
    lay = gkr.layout_frac(m)
    assert (len(rounds), len(points), len(claims), len(lambdas)) == (lay.rounds_words, lay.points_words, lay.claims_words, lay.lambdas_words)
    # the root is the sum of the fractions: root_p / root_q = sum a_p / a_q (no denominator is 0 mod r among random words)
    want = sum(p * pow(q, -1, r) for p, q in zip(a_p, a_q)) % r
    assert root_p * pow(root_q, -1, r) % r == want
    for as_bytes in (False, True):
        args = [_pack(x) if as_bytes else x for x in (rounds, points, claims, lambdas)]
        state, point, (claim_p, claim_q) = gkr.verify_fraction(field, m, root_p, root_q, state0, *args)
        assert state == final and point == points[lay.points[m - 1]:] and len(point) == m
        assert claim_p == mle_at(a_p, point, r) and claim_q == mle_at(a_q, point, r)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("m", (1, 2, 5))
def test_verifier_rejects_one_flipped_word_and_names_the_layer(field, m):
    a_p, a_q, state0, root_p, root_q, rounds, points, claims, lambdas, _ = _proof(field, m)
    lay = gkr.layout_frac(m)

    def refused(match, root_p=root_p, root_q=root_q, rounds=rounds, points=points, claims=claims, lambdas=lambdas):
        with pytest.raises(ValueError, match=match):
            gkr.verify_fraction(field, m, root_p, root_q, state0, rounds, points, claims, lambdas)

    def flipped(words, at):
        return words[:at] + [words[at] ^ 1] + words[at + 1:]

    refused(r"layer 0\b", root_p=root_p ^ 1)
    refused(r"layer 0\b", root_q=root_q ^ 1)
    for j in range(m):
        for t in range(4):   # each claim word: the layer's final check
            refused(rf"layer {j}\b", claims=flipped(claims, lay.claims[j] + t))
        refused(rf"layer {j}\b", points=flipped(points, lay.points[j] + j))   # rho_j
        if j >= 1:
            refused(rf"layer {j}\b", lambdas=flipped(lambdas, j))
        for i in range(j):
            for t in range(3):   # u_i(0) and u_i(1) fail the sum, u_i(2) the challenge derived from the row
                refused(rf"layer {j}, round {i}\b", rounds=flipped(rounds, lay.rounds[j] + 3 * i + t))
            refused(rf"layer {j}, round {i}\b", points=flipped(points, lay.points[j] + j - 1 - i))
    # word 0 of the lambdas is not part of the proof
    gkr.verify_fraction(field, m, root_p, root_q, state0, rounds, points, claims, flipped(lambdas, 0))
    # a proof that is consistent with itself, but from another transcript state
    with pytest.raises(ValueError, match=r"layer 0\b"):   # the first challenge, rho_0, is not that state's
        gkr.verify_fraction(field, m, root_p, root_q, bytes(32), rounds, points, claims, lambdas)


@pytest.mark.parametrize("field", FIELDS)
def test_logup_instance_sums_to_zero_and_one_bad_lookup_does_not(field):
    r = fiat_shamir.MODULUS[field]
    for bad in (False, True):
        a_p, a_q = logup_instance(field, bad=bad)
        assert len(a_p) == len(a_q) == 64
        root_p, root_q, rounds, points, claims, lambdas, final = prove_ref(field, a_p, a_q, bytes(32))
        lp, lq = frac_trees(a_p, a_q, r)
        assert (root_p, root_q) == (lp[6][0], lq[6][0]) and root_q != 0
        assert (root_p == 0) == (not bad)
        state, point, (claim_p, claim_q) = gkr.verify_fraction(field, 6, root_p, root_q, bytes(32), rounds, points, claims, [0] + lambdas[1:])
        assert state == final and claim_p == mle_at(a_p, point, r) and claim_q == mle_at(a_q, point, r)


def test_kernels_in_their_own_header_behind_one_slot():
    impl = _read("blaze_amd", "csrc", "ntt_impl.hip.hpp")
    eng = _read("blaze_amd", "csrc", "ntt_engine.hpp")
    assert impl.index('#include "ntt_gkr.hip.hpp"') < impl.index('#include "ntt_fgkr.hip.hpp"')
    assert impl.count("o.fgkr_tail = ") == 1 and len(re.findall(r"\(\*fgkr_tail\)\s*\(\s*hipStream_t\s+st\s*,", eng)) == 1
    assert re.search(r"constexpr\s+uint32_t\s+FGKR_TAIL_LEN\s*=\s*1u\s*<<\s*FGKR_TAIL_LOG\s*;", eng) and re.search(r"constexpr\s+int\s+FGKR_TAIL_LOG\s*=\s*8\s*;", eng)
    src = _read("blaze_amd", "csrc", "ntt_fgkr.hip.hpp")
    kernels = re.findall(r"template\s*<([^>]*)>\s*__global__[^\n;{]*?\bvoid\s+(\w+)\s*\(", src)
    assert kernels == [("class Fr", "k_fgkr_tail"), ("class Fr", "k_fgkr_claims")], kernels
    assert '#include "ntt_gkr.hip.hpp"' in src and "WHY EVERY INTERMEDIATE FITS" in src and "THE SUM OF TWO PRODUCTS" in src
    statements = _uncommented(src)
    for banned in ("atomic", "alloc", "volatile", "__threadfence", "asm", "ws", "while (true)", "for (;;)"):
        assert not re.search(rf"\b{re.escape(banned)}", statements), banned
    # the transcript is ntt_gkr.hip.hpp's: its lane layout, its constants, its one-block step; the two-block step is this header's
    for used in ("GkrKeccakLane", "gkr_pack<Fr>(", "gkr_challenge(", "gkr_absorb(", "fgkr_absorb2(", "GKR_KECCAK_RC[round]"):
        assert used in statements, used
    assert "ntt_fs" not in statements and "GKR_KECCAK_RC[24]" not in statements
    # every lane of the one block reaches every barrier: nothing returns out of the kernels, and wave 0's transcript holds none
    body = statements[statements.index("void k_fgkr_tail("): statements.index("void k_fgkr_claims(")]
    assert "return" not in body and body.count("__syncthreads()") >= 6
    lines = body.split("\n")
    heads = [k for k, ln in enumerate(lines) if ln.strip() == "if (wave0) {"]
    assert len(heads) == 3 and body.count("wave0)") == 3   # lambda, a row, the claims
    for k in heads:
        indent = lines[k][:len(lines[k]) - len(lines[k].lstrip())]
        end = next(e for e in range(k + 1, len(lines)) if lines[e] == indent + "}")
        assert "__syncthreads" not in "\n".join(lines[k:end]) and "absorb" in "\n".join(lines[k:end])
    # the state is read once and stored once; no table word, no weight word goes back to memory
    assert body.count("g.state") == 2 and not re.search(r"fp_store\(\s*(gp|gq|g\.tree_p|g\.tree_q|g\.a_p|g\.a_q|g\.weight)\b", body)
    claims = statements[statements.index("void k_fgkr_claims("): statements.index("int ntt_fgkr_tail_t(")]
    assert re.findall(r"fp_store\(\s*([\w.]+)", claims) == ["g.claims"]
    # the new text of ntt.hip does not speak of the grand product's kernels
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    assert "k_gkr_" not in ntt[ntt.index(f"int {NAME}(") - 2000:ntt.index("int blz_ntt_last_kernel_ms(")]


def test_entry_point_checks_first_in_the_documented_order():
    ntt = _read("blaze_amd", "csrc", "ntt.hip")
    body = function_body(ntt, f"int {NAME}(")
    for once in ("call.begin()", "call.live_length(", "call.resolve(", "call.enqueue(", "call.device_range(", "NttVecCall::words_meet(", "h->ops->vec_mle_eq(",
                 "h->ops->sumcheck_gate(", "h->ops->gate_eval("):
        assert body.count(once) == 1, once
    assert body.count("h->ops->zerocheck_gate(") == 2 and body.count("ntt_fs_absorb(") == 3 and body.count("h->ops->fgkr_tail(") == 3
    order = ['"null handle"', "unknown GKR flags", "tree_p is NULL", "tree_q is NULL", "a_p is NULL", "a_q is NULL", "d_weight is NULL", "d_state is NULL",
             "d_rounds is NULL", "d_points is NULL", "d_claims is NULL", "d_lambdas is NULL", "call.live_length(", "call.begin()", "call.resolve(",
             "a tree over len", "the leaves are folded in place", "call.device_range(", "NttVecCall::words_meet(", "call.enqueue("]
    at = [body.index(s) for s in order]
    assert at == sorted(at), list(zip(order, at))
    # the ranges are checked in the documented order
    names = re.findall(r'\{("d_\w+"|oname\[\d\]), ', body[body.index("const Range rg["):body.index("call.device_range(")])
    assert names == ["oname[0]", "oname[1]", "oname[2]", "oname[3]", '"d_weight"', '"d_state"', '"d_rounds"', '"d_points"', '"d_claims"', '"d_lambdas"'], names
    assert 'oname[4] = {"tree_p", "tree_q", "a_p", "a_q"}' in body
    # nothing is launched ahead of the enqueue, and nothing waits for the device or copies through the host
    head = body[:body.index("call.enqueue(")]
    for launched in ("h->ops->", "ntt_fs_absorb(", "hipLaunchKernelGGL"):
        assert launched not in head, launched
    for waits in ("hipStreamSynchronize", "sync_stream_bounded", "hipMemcpy", "hipEventSynchronize", "hipLaunchKernelGGL"):
        assert waits not in body, waits
    # the grand product is as it was
    prod = function_body(ntt, f"int {GKR}(")
    assert "fgkr" not in prod and "BLZ_TREE_FRAC is not built" in prod


def test_documented_where_the_other_ops_are():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "HISTORY.md"):
        assert "gkr_prove_frac" in _read(doc), doc
    design = _read("DESIGN.md")
    assert "**One-call fraction GKR**" in design and design.index("**One-call GKR**") < design.index("**One-call fraction GKR**")
    section = design[design.index("**One-call fraction GKR**"):]
    for said in ("k_fgkr_tail", "FGKR_TAIL_LEN", "256", "72 KiB", "VGPR", "ntt_gkr_frac_timing.py", "ntt_gkr_frac.json", "Out of scope", "BLZ_MLE_LOW", "lambda"):
        assert said in section, said
    old = design[design.index("**One-call GKR**"):design.index("**One-call fraction GKR**")]
    assert "Out of scope" in old and "BLZ_TREE_FRAC" in old
    assert os.path.exists(os.path.join(ROOT, "tools", "ntt_gkr_frac_timing.py"))


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    notes = disassemble_library(LIB, "llvm-readelf", "--notes")
    # (a kernel's map is sorted by key: .group_segment_fixed_size comes before .name)
    lds = {n: int(v) for v, n in re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\s+\.group_segment_fixed_size:).*\n)*?\s+\.name:\s+(\S+)", notes)}
    return kernel_vgprs(LIB), kernel_scratch(LIB), lds, disassemble_library(LIB)


VGPR_CAP = 128   # the next occupancy step: four waves per SIMD, test_ntt_gkr.py's rule ("One-call fraction GKR")
LDS_MIN, LDS_CAP = 36 * 1024, 64 * 1024   # four tables of 256 words and a weight of 128; what a static allocation may have


def test_three_tails_and_three_claims_without_scratch_within_the_caps(code):
    vgprs, scratch, lds, text = code
    names = sorted(n for n in vgprs if re.match(r"_ZN3blz\d+k_fgkr_", n))
    print({n: (vgprs[n], scratch[n], lds[n]) for n in names})
    assert names == sorted(f"_ZN3blz{k}INS_{f}EEEvNS_11NttFgkrTailE" for k in ("11k_fgkr_tail", "13k_fgkr_claims") for f in MANGLED), names
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= VGPR_CAP, (n, vgprs[n])
        ins = function_instructions(text, n)
        if "k_fgkr_tail" in n:
            assert LDS_MIN <= lds[n] <= LDS_CAP, lds[n]
            assert count(ins, "v_mad_u64_u32") >= 256, n
            assert count(ins, "ds_bpermute_b32") >= 18 and count(ins, "s_barrier") >= 6, n
        else:
            assert lds[n] == 0, n
