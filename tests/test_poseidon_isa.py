"""The Poseidon kernels of the shipped gfx950 code object against the figures DESIGN.md section 8 gives for them: no scratch,
a register count inside the three-waves-per-SIMD budget (168 VGPRs), and a v_mad_u64_u32 count equal to the section's formula -
so the issue fraction tools/poseidon_timing.py reports is priced from the code, not from a guess.

Formula (static count of k_poseidon_hash<field, t>; the round loop's body appears once):
    MUL = 81 + QM, SQR = 45 + QM, QM = 81 quotient products of a reduction, minus the 9 by the modulus's lowest limb where that
    limb is 1 (BLS12-381 / BLS12-377 Fr: the product is an addition)
    count = 3 MUL (input conversion, x^4 x, output conversion) + 2 SQR (x^2, x^4) + 81 t + QM ceil(t / 6)   (+ address arithmetic)"""
import os
import re

import pytest

from isa_util import count, disassemble_library, function_instructions, kernel_vgprs, loops, tools_available

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

HASH = "_ZN3blz15k_poseidon_hashINS_{n}{f}ELi{t}EEEvNS_13PoseidonWidthENS_11PoseidonJobE"
FIELDS = {"Fr_BLS377_RR": 72, "Fr_BLS381_RR": 72, "Fr_BN254_RR": 81}     # QM
TOL = 8   # test_isa_counts.py's tolerance: 64-bit address arithmetic also compiles to v_mad_u64_u32
VGPR_BUDGET = 168   # three waves per SIMD (512 / 168, allocation granule 8)


def static_mads(qm, t):
    return 3 * (81 + qm) + 2 * (45 + qm) + 81 * t + qm * ((t + 5) // 6)


def wave_mads_per_permutation(qm, t, rf, rp):
    """what a WAVE issues for the 64 // t hashes it holds: every round pays the S-box and a matrix row,
    whatever the round's kind (in a partial round the lanes without an S-box wait for lane 0's)"""
    return 2 * (81 + qm) + (rf + rp) * ((81 + qm) + 2 * (45 + qm) + 81 * t + qm * ((t + 5) // 6))


@pytest.fixture(scope="module")
def code():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    text = disassemble_library(LIB)
    notes = disassemble_library(LIB, "llvm-readelf", "--notes")
    scratch = {n: int(v) for n, v in re.findall(
        r"^\s+\.name:\s+(\S+)\n(?:(?!\s+\.name:).*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", notes, re.M)}
    return text, kernel_vgprs(LIB), scratch


def test_every_poseidon_kernel_is_there_without_scratch_and_inside_the_budget(code):
    _, vgprs, scratch = code
    names = [n for n in vgprs if "poseidon" in n]
    want = {HASH.format(n=len(f), f=f, t=t) for f in FIELDS for t in range(2, 17)}
    want |= {f"_ZN3blz15k_poseidon_prepINS_{len(f)}{f}EEEvPKjPjj" for f in FIELDS}
    assert set(names) == want, sorted(set(names) ^ want)
    for n in names:
        assert scratch[n] == 0, (n, scratch[n])
        assert vgprs[n] <= VGPR_BUDGET, (n, vgprs[n])


@pytest.mark.parametrize("field", sorted(FIELDS))
@pytest.mark.parametrize("t", [2, 3, 6, 7, 9, 12, 13, 16])
def test_multiply_add_count_is_the_formula(code, field, t):
    text, _, _ = code
    ins = function_instructions(text, HASH.format(n=len(field), f=field, t=t))
    mads = count(ins, "v_mad_u64_u32")
    want = static_mads(FIELDS[field], t)
    print(f"{field} t = {t}: {mads} multiply-adds, formula {want}")
    assert want <= mads <= want + TOL, (mads, want)
    # the round loop is ONE loop (not unrolled, not versioned by round kind): its body holds everything but the two conversions
    big = [body for _, _, body in loops(ins) if count(body, "v_mad_u64_u32") > 100]
    assert big, "no round loop found"
    inner = count(min(big, key=len), "v_mad_u64_u32")
    assert want - 2 * (81 + FIELDS[field]) <= inner <= want - 2 * (81 + FIELDS[field]) + TOL, (inner, want)


def test_headline_figures():
    """the numbers DESIGN.md quotes for the fixture's (8, 57) rounds on BLS12-381"""
    assert static_mads(72, 12) == 1809 and static_mads(72, 9) == 1566
    assert wave_mads_per_permutation(72, 12, 8, 57) == 98001 and wave_mads_per_permutation(72, 9, 8, 57) == 82206
