"""The MSM tail's kernels in the shipped code object (no device): which of them every field instantiation has - the fold /
reduce / finish kernels of the laws the field has (tests/msm_tail_ref.py LAWS) and no others - and what each costs in VGPRs
and private segment (scratch) bytes.  The figures are those of the build BEFORE the kernels became wrappers around one body
per algorithm (reduce_segment, horner_walk, fold_units over the group-law policies of ec_law.hip.hpp): the rewrite was
required to leave every kernel's resources where they were, and a later change that moves one should do so knowingly.
Moved since, BLS12-377 only: k_combine_buckets_wave, k_merge_buckets, k_reduce_level0_rr and k_reduce_level_rr, when the
reduced-radix doublings of the curve with a group of even order learnt to answer infinity for a point of order two
(ec_rr.hip.hpp RR_EVEN_ORDER); the row kernels, whose test sits behind the doubling chain, and every other field kept theirs."""
import os
import re

import pytest

from isa_util import ROOT, kernel_scratch, kernel_vgprs, tools_available
from msm_tail_ref import LAWS

LIB = os.environ.get("BLAZE_HIP_LIB") or os.path.join(ROOT, "blaze_amd", "lib", "libblaze_hip.so")

# field class of (curve, 32-bit-limb build) in LAWS
FIELD = {("BLS377", 0): "BLS377", ("BLS381", 0): "BLS381", ("BN254", 0): "BN254", ("BN254", 1): "BN254_W32"}
TAIL = re.compile(r"^_ZN3blz\d+(k_(?:reduce_level|finish|combine_buckets|fold_hot|merge_buckets)[a-z0-9_]*)"
                  r"INS_\d+Fq_(BLS377|BLS381|BN254_W32|BN254)E(?:Lb([01])E)?EEv")

# kernel: (.vgpr_count, .private_segment_fixed_size)
COST = {
    "BLS377": {
        "k_combine_buckets": (168, 688),
        "k_combine_buckets_row<false>": (30, 0),
        "k_combine_buckets_row<true>": (30, 0),
        "k_combine_buckets_wave": (248, 464),
        "k_finish_row": (136, 256),
        "k_fold_hot": (256, 512),
        "k_fold_hot_row": (40, 0),
        "k_merge_buckets": (248, 464),
        "k_reduce_level0_quad": (256, 24),
        "k_reduce_level0_rr": (256, 496),
        "k_reduce_level_row<false>": (46, 0),
        "k_reduce_level_row<true>": (34, 0),
        "k_reduce_level_rr": (256, 484),
    },
    "BLS381": {
        "k_combine_buckets": (168, 672),
        "k_combine_buckets_row<false>": (30, 0),
        "k_combine_buckets_row<true>": (30, 0),
        "k_combine_buckets_wave": (232, 464),
        "k_finish_row": (100, 256),
        "k_fold_hot": (253, 464),
        "k_fold_hot_row": (40, 0),
        "k_merge_buckets": (232, 464),
        "k_reduce_level0_quad": (256, 32),
        "k_reduce_level0_rr": (256, 464),
        "k_reduce_level_row<false>": (46, 0),
        "k_reduce_level_row<true>": (34, 0),
        "k_reduce_level_rr": (256, 480),
    },
    "BN254": {
        "k_combine_buckets": (148, 304),
        "k_combine_buckets_wave": (148, 304),
        "k_finish": (171, 176),
        "k_fold_hot": (175, 304),
        "k_merge_buckets": (148, 304),
        "k_reduce_level0_quad": (171, 0),
        "k_reduce_level0_rr": (174, 304),
        "k_reduce_level_rr": (245, 0),
    },
    "BN254_W32": {
        "k_combine_buckets": (142, 272),
        "k_finish": (104, 544),
        "k_merge_buckets": (145, 272),
        "k_reduce_level<false>": (104, 672),
        "k_reduce_level<true>": (174, 272),
    },
}


def kernels_of(rr, row):
    """The tail kernels of a field with these laws (run_accumulate_t / run_reduce_t instantiate nothing else)."""
    out = {"k_combine_buckets", "k_merge_buckets"}
    out |= {"k_combine_buckets_wave", "k_fold_hot", "k_reduce_level0_rr", "k_reduce_level0_quad", "k_reduce_level_rr"} if rr \
        else {"k_reduce_level<true>", "k_reduce_level<false>"}
    out |= {"k_combine_buckets_row<true>", "k_combine_buckets_row<false>", "k_fold_hot_row", "k_reduce_level_row<true>",
            "k_reduce_level_row<false>", "k_finish_row"} if row else {"k_finish"}
    return out


@pytest.fixture(scope="module")
def shipped():
    if not tools_available():
        pytest.skip("ROCm LLVM tools not installed")
    vgprs, scratch = kernel_vgprs(LIB), kernel_scratch(LIB)
    out = {f: {} for f in FIELD.values()}
    for name in vgprs:
        m = TAIL.match(name)
        if m:
            flag = "" if m.group(3) is None else "<true>" if m.group(3) == "1" else "<false>"
            out[m.group(2)][m.group(1) + flag] = (vgprs[name], scratch[name])
    return out


@pytest.mark.parametrize("key", sorted(LAWS))
def test_a_field_has_the_tail_kernels_of_its_laws_and_no_others(shipped, key):
    rr, row = LAWS[key]
    have = set(shipped[FIELD[key]])
    assert have == kernels_of(rr, row)
    assert have == set(COST[FIELD[key]])
    if not rr:
        assert not [k for k in have if re.search(r"rr|quad|wave|hot", k)]
    if not row:
        assert not [k for k in have if "row" in k]


@pytest.mark.parametrize("key", sorted(LAWS))
def test_tail_kernels_keep_their_vgprs_and_scratch(shipped, key):
    print(shipped[FIELD[key]])
    assert shipped[FIELD[key]] == COST[FIELD[key]]
