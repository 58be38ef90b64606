"""The optimised partial rounds, the part that needs no device: the new entry point in every layer, and the algebra - the
derivation and the permutation on the derived tables in Python integers (tests/poseidon_sparse_ref.py) against the dense
definition (tests/poseidon_ref.py)."""
import ctypes as C
import os
import random
import re

import pytest

import blaze_amd
import poseidon_ref as R
import poseidon_sparse_ref as S
from blaze_amd._lib import AUX_EXPORTED_SYMBOLS, EXPORTED_SYMBOLS
from blaze_amd.ingo_hash import PoseidonClient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "blz_poseidon_prepare_round_plan"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_entry_point_in_every_layer():
    assert re.search(rf"\bint\s+{NAME}\s*\(\s*blz_poseidon\s*\*\s*h\s*,\s*uint32_t\s+out\[2\]\s*\)", _read("include", "blaze_hip.h"))
    assert NAME in EXPORTED_SYMBOLS and getattr(C.CDLL(blaze_amd._lib.LIB_PATH), NAME) is not None
    assert callable(getattr(PoseidonClient, "prepare_round_plan"))
    assert NAME in _read("include", "blaze.hpp") and "prepare_round_plan()" in _read("include", "blaze.hpp")
    assert re.search(rf"pub fn {NAME}\(h: \*mut BlzPoseidon, out: \*mut u32\) -> c_int;", _read("rust", "src", "driver_client", "hip_ffi.rs"))
    assert "pub fn prepare_round_plan(&self)" in _read("rust", "src", "ingo_hash", "poseidon_api.rs")
    assert "prepare_round_plan" in _read("INTEGRATION.md")
    assert "blz_test_poseidon_hash_plan" in AUX_EXPORTED_SYMBOLS and getattr(blaze_amd.aux(), "blz_test_poseidon_hash_plan") is not None
    assert "blz_test_poseidon_hash_plan" not in EXPORTED_SYMBOLS


def test_null_handle_is_refused():
    out = (C.c_uint32 * 2)()
    assert blaze_amd.lib().blz_poseidon_prepare_round_plan(None, out) == 4
    assert blaze_amd.lib().blz_poseidon_prepare_round_plan(None, None) == 4


def random_block(rng, r, t, rf, rp):
    return dict(t=t, rf=rf, rp=rp, tag=rng.randrange(r), rc=[[rng.randrange(r) for _ in range(t)] for _ in range(rf + rp)],
                mds=[[rng.randrange(r) for _ in range(t)] for _ in range(t)])


@pytest.mark.parametrize("field", sorted(R.MODULUS))
@pytest.mark.parametrize("rounds", [(8, 57), (8, 5), (2, 1), (2, 0)])
def test_model_equals_the_dense_definition(field, rounds):
    """random NON-SYMMETRIC matrices (a Cauchy matrix would hide a swap of the sparse row and column), random states, 0 and r - 1"""
    r = R.MODULUS[field]
    rng = random.Random(f"{field}{rounds}")
    for t in (2, 3, 9, 12, 16):
        blk = random_block(rng, r, t, *rounds)
        tables = S.derive(blk, r)
        assert len(tables["sparse"]) == len(tables["rc"]) == rounds[1]
        for state in ([0] * t, [r - 1] * t, [rng.randrange(r) for _ in range(t)]):
            assert S.permute(state, blk, r, tables) == R.permute(state, blk, r), (t, rounds)
        x = [rng.randrange(r) for _ in range(t - 1)]
        assert S.hash_fixed(x, blk, r, tables) == R.hash_fixed(x, blk, r)


def test_model_refuses_a_singular_lower_right_block():
    """two equal rows in M without row 0 and column 0: no plan - though M itself can still be invertible; with no partial round
    there is nothing to derive and the width is admitted"""
    r = R.MODULUS["BLS381"]
    rng = random.Random(5)
    blk = random_block(rng, r, 4, 8, 5)
    blk["mds"][3][1:] = blk["mds"][2][1:]
    full = S.invert(blk["mds"], r)                      # M is invertible
    assert S.mat_mul(full, blk["mds"], r) == S.identity(4)
    with pytest.raises(S.Singular):
        S.derive(blk, r)
    blk.update(rp=0, rc=blk["rc"][:8])
    assert S.derive(blk, r)["pre"] == blk["mds"]
    assert S.permute([1, 2, 3, 4], blk, r) == R.permute([1, 2, 3, 4], blk, r)
