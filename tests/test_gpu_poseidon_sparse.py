"""The optimised partial rounds of the Poseidon tree client on the MI355X: k_hades_hash on tables derived on
the device against the definition kernel (dense rounds, 8 x 32-bit arithmetic) and against Python; the self-check, its refusal, the
switch, and the lazy preparation.  Every comparison is bit for bit: the optimised rounds change no byte of any record."""
import ctypes as C
import random

import pytest

import blaze_amd
import poseidon_fixtures
import poseidon_ref as R
from blaze_amd import DeviceBuffer
from blaze_amd._lib import buf_ptr, check
from blaze_amd.driver_client import DriverClient
from blaze_amd.ingo_hash import Hash, PoseidonClient, PoseidonInitializeParameters, PoseidonResult, TreeMode

pytestmark = pytest.mark.gpu

FIXTURE = poseidon_fixtures.path("bls381_t9_t12")
WIDTHS = (2, 3, 6, 7, 9, 12, 13, 16)      # every shape of ceil(t / 6) and of 64 mod t
ON, REFUSED = 1, 2

_cache = {}


def memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def block_spans(words):
    """[(first word, one past the last word)] of every block of a stream"""
    spans, pos = [], 3
    for _ in range(words[2]):
        t, _alpha, rf, rp = words[pos:pos + 4]
        end = pos + 5 + t * (rf + rp) + t * t
        spans.append((pos, end))
        pos = end
    return spans


def small_stream_extended(field):
    """the <field>_small stream (t = 3, 9, 12 with (8, 5) rounds) plus the tool's blocks for the widths it lacks, every matrix
    replaced by random elements: (words, blocks)"""
    def make():
        small = R.read_instruction_words(poseidon_fixtures.path(f"{field.lower()}_small"))
        have = set(R.parse_stream(small)[0])
        extra = poseidon_fixtures.tool().generate(field, [(t, 8, 5) for t in WIDTHS if t not in have])
        words = small[:2] + [small[2] + extra[2]]
        for src in (small, extra):
            for a, b in block_spans(src):
                words += src[a:b]
        if len(words) % 2:
            words.append(0)
        words = poseidon_fixtures.with_random_matrices(words, R.MODULUS[field], 61)
        return words, R.parse_stream(words)[0]
    return memo(("small", field), make)


def el_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def hash_plan(field, wb, t, inputs):
    """blz_test_poseidon_hash_plan: (state, digests as integers)"""
    n = len(inputs)
    raw = bytearray(el_bytes([x for row in inputs for x in row]))
    dig = bytearray(32 * n)
    state = C.c_uint32(0)
    check(blaze_amd.aux().blz_test_poseidon_hash_plan(0, R.FIELD_ID[field], buf_ptr(wb)[0], len(wb), t, buf_ptr(raw)[0], buf_ptr(dig)[0], n,
                                                      C.byref(state)))
    return state.value, [int.from_bytes(dig[32 * i: 32 * i + 32], "little") for i in range(n)]


def inputs_for(t, n, r, seed):
    rng = random.Random(seed)
    rows = [[rng.randrange(r) for _ in range(t - 1)] for _ in range(n)]
    rows[0] = [0] * (t - 1)
    rows[1] = [r - 1] * (t - 1)
    rows[2] = [(1 << 256) - 1] * (t - 1)
    rows[-1][0] = r + 1                                  # the ragged tail holds a word >= r too
    return rows


# ---------------------------------------------------------------------------------------------- 1. / 2. the kernel

@pytest.mark.parametrize("field", ["BLS377", "BLS381", "BN254"])
@pytest.mark.parametrize("t", WIDTHS)
def test_plan_kernel_equals_definition_kernel(gpu, field, t):
    """several waves plus a ragged tail per width through k_hades_hash (tables derived on the device) and through the definition
    kernel: every digest equal.  Random matrices: a Cauchy matrix is symmetric and would hide a swap of the sparse row and column."""
    r = R.MODULUS[field]
    words, blocks = small_stream_extended(field)
    blk = blocks[t]
    assert t == 2 or any(blk["mds"][i][j] != blk["mds"][j][i] for i in range(t) for j in range(i))
    wb = R.words_bytes(words)
    n = 3 * (64 // t) + 1
    rows = inputs_for(t, n, r, 100 * t + len(field))
    state, got = hash_plan(field, wb, t, rows)
    assert state == ON
    states = bytearray(el_bytes([x for row in rows for x in [blk["tag"]] + row]))
    out = bytearray(len(states))
    check(blaze_amd.aux().blz_test_poseidon_permute(0, R.FIELD_ID[field], buf_ptr(wb)[0], len(wb), t, buf_ptr(states)[0], buf_ptr(out)[0], n))
    want = [int.from_bytes(out[32 * (i * t + 1): 32 * (i * t + 2)], "little") for i in range(n)]
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, f"{len(bad)} of {n} digests differ, first at input {bad[:5]}"
    assert got[5] == R.hash_fixed(rows[5], blk, r)       # ... and the definition kernel is not wrong the same way


@pytest.mark.parametrize("rounds", [(2, 0), (2, 1), (2, 2)])
@pytest.mark.parametrize("t", [3, 12])
def test_round_numbers_the_trees_never_use(gpu, t, rounds):
    """no partial round (nothing to derive), one (the pre-sparse matrix is Mh M), two; a first half of one full round"""
    r = R.MODULUS["BLS381"]
    words = poseidon_fixtures.with_random_matrices(poseidon_fixtures.tool().generate("BLS381", [(t,) + rounds]), r, 62)
    blk = R.parse_stream(words)[0][t]
    rows = inputs_for(t, 64 // t + 2, r, 7 * t + rounds[1])
    state, got = hash_plan("BLS381", R.words_bytes(words), t, rows)
    assert state == ON
    assert got == [R.hash_fixed(row, blk, r) for row in rows]


# ---------------------------------------------------------------------------------------------- 3. - 7. the tree client

def client():
    return PoseidonClient(Hash.Poseidon, DriverClient(0), field="BLS381")


def n_inputs(h, mode):
    return (11 if mode == TreeMode.TreeC else 1) * 8 ** (h - 1)


def py_tree(words, h, mode, seed):
    def make():
        r = R.MODULUS["BLS381"]
        rng = random.Random(seed)
        el = [rng.randrange(r) for _ in range(n_inputs(h, mode))]
        return el, R.tree(el, h, int(mode), R.parse_stream(words)[0], r)
    return memo(("tree", hash(tuple(words)), h, int(mode), seed), make)


def fixture_words():
    return memo("fixture", lambda: R.read_instruction_words(FIXTURE))


def as_dict(results):
    out = {(x.layer_id, x.hash_id): int.from_bytes(x.hash_byte, "little") for x in results}
    assert len(out) == len(results)
    return out


def feed(cl, el, chunks=None):
    data, pos, k = el_bytes(el), 0, 0
    while pos < len(el):
        c = len(el) if chunks is None else chunks[k % len(chunks)]
        cl.set_data(data[32 * pos: 32 * (pos + c)])
        pos, k = pos + c, k + 1


def plan_of(info):
    return int(info["optimised_partial_rounds"]), info["round_plan_check"]


@pytest.mark.parametrize("mode", [TreeMode.TreeC, TreeMode.TreeD])
def test_prepared_trees_equal_python(gpu, mode):
    """the (8, 57) fixture: prepare -> in force, self-check equal; every record of a tree fed in one call and in ragged chunks"""
    h = 3
    el, want = py_tree(fixture_words(), h, mode, 71)
    n = R.num_records(h, int(mode))
    cl = client()
    cl.initialize(PoseidonInitializeParameters(h, mode, FIXTURE))
    before = cl.info()
    assert plan_of(before) == (0, 0)
    assert plan_of(cl.prepare_round_plan()) == (1, ON)
    info = cl.info()
    assert plan_of(info) == (1, ON) and info["device_bytes"] > before["device_bytes"]       # the derived tables count
    assert plan_of(cl.prepare_round_plan()) == (1, ON)                                      # again: nothing to do
    feed(cl, el)
    assert as_dict(cl.result(n)) == want
    feed(cl, el, chunks=[1, 10, 12, 7, 350, 3, 93, 2])
    assert as_dict(cl.result(n)) == want
    assert plan_of(cl.info()) == (1, ON)
    cl.close()


def test_plan_is_prepared_under_the_first_tree(gpu):
    """no prepare call: the first tree's first launch finds the plan derived and checked"""
    h, mode = 3, TreeMode.TreeC
    el, want = py_tree(fixture_words(), h, mode, 71)
    cl = client()
    cl.initialize(PoseidonInitializeParameters(h, mode, FIXTURE))
    assert plan_of(cl.info()) == (0, 0)
    feed(cl, el)
    assert as_dict(cl.result(R.num_records(h, int(mode)))) == want
    assert plan_of(cl.info()) == (1, ON)
    assert 0 < cl.last_kernel_ms() < 10_000
    cl.close()


def test_singular_block_is_refused_and_hashed_densely(gpu):
    """two equal rows in the t = 9 matrix without its row 0 and column 0: refused, never an error - the dense rounds give the records"""
    h, mode = 3, TreeMode.TreeD
    words = list(fixture_words())
    (a9, b9), _ = block_spans(words)
    assert words[a9] == 9
    m = b9 - 81
    words[m + 9 * 4 + 1: m + 9 * 5] = words[m + 9 * 3 + 1: m + 9 * 4]
    el, want = py_tree(words, h, mode, 72)
    cl = client()
    cl.initialize_words(h, mode, R.words_bytes(words))
    assert plan_of(cl.prepare_round_plan()) == (0, REFUSED)
    feed(cl, el)
    assert as_dict(cl.result(R.num_records(h, int(mode)))) == want
    assert plan_of(cl.info()) == (0, REFUSED)
    # ... and the kernel's own hook says the same for that width, with no digests
    state, _ = hash_plan("BLS381", R.words_bytes(words), 9, inputs_for(9, 8, R.MODULUS["BLS381"], 3))
    assert state == REFUSED
    cl.close()


def test_switch_initialize_and_reset(gpu):
    h, mode = 3, TreeMode.TreeD
    el, want = py_tree(fixture_words(), h, mode, 71)
    n = R.num_records(h, int(mode))
    cl = client()
    cl.initialize(PoseidonInitializeParameters(h, mode, FIXTURE))
    assert plan_of(cl.prepare_round_plan()) == (1, ON)
    held = cl.info()["device_bytes"]
    cl.set_round_plan(False)
    assert plan_of(cl.info()) == (0, ON)                 # out of force at once; the tables stay
    assert plan_of(cl.prepare_round_plan()) == (0, ON)   # with the setting at 0: does nothing
    feed(cl, el)
    assert as_dict(cl.result(n)) == want
    cl.set_round_plan(True)
    assert plan_of(cl.info()) == (1, ON) and cl.info()["device_bytes"] == held
    feed(cl, el)
    assert as_dict(cl.result(n)) == want
    cl.reset()
    assert plan_of(cl.info()) == (1, ON)                 # reset keeps them
    cl.initialize(PoseidonInitializeParameters(h, mode, FIXTURE))
    assert plan_of(cl.info()) == (0, 0)                  # initialize discards tables and state
    cl.close()
    fresh = client()
    with pytest.raises(blaze_amd.DriverClientError) as ei:
        fresh.prepare_round_plan()                       # before initialize
    assert ei.value.variant == "InvalidPrimitiveParam"
    fresh.close()


def test_every_node_of_a_tree_under_the_plan(gpu):
    """TreeC h = 5 (4681 nodes) with the plan in force: every node re-hashed from its children by the definition kernel"""
    h, mode = 5, TreeMode.TreeC
    wb = R.words_bytes(fixture_words())
    n_in, n_rec = n_inputs(h, mode), R.num_records(h, int(mode))
    d_in = DeviceBuffer(0, 32 * n_in)
    check(blaze_amd.aux().blz_synth_field_elements(0, d_in.ptr, n_in, 4247))
    cl = client()
    cl.initialize(PoseidonInitializeParameters(h, mode, FIXTURE))
    assert plan_of(cl.prepare_round_plan()) == (1, ON)
    cl.set_data(d_in)
    cl.wait_result()
    d_rec = DeviceBuffer(0, 64 * n_rec)
    cl.tree_device(d_rec)
    out = (C.c_uint64 * 2)()
    check(blaze_amd.aux().blz_test_poseidon_tree_check(0, 1, buf_ptr(wb)[0], len(wb), int(mode), h, d_in.ptr, d_rec.ptr, out))
    assert out[0] == n_rec and out[1] == 0, f"{out[1]} of {out[0]} nodes differ from the definition kernel"
    root = PoseidonResult.parse_poseidon_hash_results(d_rec.download(64, 64 * (n_rec - 1)))[0]
    assert (root.layer_id, root.hash_id) == (h - 1, 0)
    d_in.free()
    d_rec.free()
    cl.close()
