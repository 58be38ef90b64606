"""The kernels of the optimised partial rounds in the shipped gfx950 code object against the figures DESIGN.md section 8 gives
for them: every instantiation present, no scratch, a register count inside the three-waves-per-SIMD budget (168 VGPRs), and the
partial-round loop's v_mad_u64_u32 count equal to the section's formula - and below a dense round's.  Counts only.

Formula (the body of the partial-round loop of k_hades_hash<field, t>, whatever t):
    2 SQR (y^2, y^4) + 2 MUL (lane 0: y^4 y | lane e: U_e y;  K_e y^5) + RD
    MUL = 81 + QM, SQR = 45 + QM as in test_poseidon_isa.py; RD = 9, the quotient-digit step that brings the sums below 2r again
    (rr_reduce2m): one product per 29-bit limb of r - the compiler turns those with a limb that is 0, 1 or a power of two into
    shifts, so the count may also fall short of the formula by a few; the tolerance is two-sided here
against the dense round's MUL + 2 SQR + 81 t + QM ceil(t / 6)."""
import os
import re

import pytest

from isa_util import count, disassemble_library, function_instructions, kernel_vgprs, loops, tools_available

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

HASH = "_ZN3blz12k_hades_hashINS_{n}{f}ELi{t}EEEvNS_13PoseidonWidthENS_9HadesPlanENS_11PoseidonJobE"
DERIVE = "_ZN3blz14k_hades_deriveINS_{n}{f}EEEvPKjiiiPjS4_"
FIELDS = {"Fr_BLS377_RR": 72, "Fr_BLS381_RR": 72, "Fr_BN254_RR": 81}     # QM
RD = 9
TOL = 8             # test_isa_counts.py's tolerance: 64-bit address arithmetic also compiles to v_mad_u64_u32
VGPR_BUDGET = 168   # three waves per SIMD (512 / 168, allocation granule 8)


def partial_round_mads(field):
    qm = FIELDS[field]
    return 2 * (45 + qm) + 2 * (81 + qm) + RD


def dense_round_mads(qm, t):
    return (81 + qm) + 2 * (45 + qm) + 81 * t + qm * ((t + 5) // 6)


def wave_mads_per_permutation(field, t, rf, rp):
    """what a wave issues for its 64 // t hashes under the plan: two conversions, R_F full rounds with
    three products per reduction (and the quotient-digit step where a row has more than one group), R_P partial rounds"""
    qm = FIELDS[field]
    full = (81 + qm) + 2 * (45 + qm) + 81 * t + qm * ((t + 2) // 3) + (RD if t > 3 else 0)
    return 2 * (81 + qm) + rf * full + rp * partial_round_mads(field)


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    text = disassemble_library(LIB)
    notes = disassemble_library(LIB, "llvm-readelf", "--notes")
    scratch = {n: int(v) for n, v in re.findall(
        r"^\s+\.name:\s+(\S+)\n(?:(?!\s+\.name:).*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", notes, re.M)}
    return text, kernel_vgprs(LIB), scratch


def test_every_instantiation_is_there_without_scratch_and_inside_the_budget(code):
    _, vgprs, scratch = code
    want = {HASH.format(n=len(f), f=f, t=t) for f in FIELDS for t in range(2, 17)}
    assert len(want) == 45 and want <= set(vgprs), sorted(want - set(vgprs))
    want |= {DERIVE.format(n=len(f) - 3, f=f[:-3]) for f in FIELDS}
    assert want <= set(vgprs), sorted(want - set(vgprs))
    for n in sorted(want):
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= VGPR_BUDGET, (n, vgprs[n])


@pytest.mark.parametrize("field", sorted(FIELDS))
@pytest.mark.parametrize("t", [2, 3, 6, 7, 9, 12, 13, 16])
def test_partial_round_loop_is_the_formula_and_below_a_dense_round(code, field, t):
    text, _, _ = code
    ins = function_instructions(text, HASH.format(n=len(field), f=field, t=t))
    # the loops that hold products: the full rounds' (one body for all three full phases), the partial rounds', and the phase
    # loop around both.  The partial rounds' is the one whose count does not grow with t: the smallest
    big = [body for _, _, body in loops(ins) if count(body, "v_mad_u64_u32") > 100]
    assert big, "no round loop found"
    inner = count(min(big, key=lambda b: count(b, "v_mad_u64_u32")), "v_mad_u64_u32")
    want = partial_round_mads(field)
    dense = dense_round_mads(FIELDS[field], t)
    print(f"{field} t = {t}: partial-round loop {inner} multiply-adds, formula {want}; a dense round {dense}")
    assert want - TOL <= inner <= want + TOL, (inner, want)
    assert inner < dense, (inner, dense)


def test_headline_figures():
    """the numbers DESIGN.md quotes for the fixture's (8, 57) rounds on BLS12-381"""
    assert partial_round_mads("Fr_BLS381_RR") == 549 and partial_round_mads("Fr_BN254_RR") == 585
    assert dense_round_mads(72, 12) == 1503 and dense_round_mads(72, 9) == 1260
    assert wave_mads_per_permutation("Fr_BLS381_RR", 12, 8, 57) == 44847 and wave_mads_per_permutation("Fr_BLS381_RR", 9, 8, 57) == 42327
