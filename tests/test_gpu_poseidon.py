"""The Poseidon tree client on the MI355X, against tests/poseidon_ref.py (textbook Python) and the definition kernel of the aux
library (blz_test_poseidon_permute: dense rounds on the 8 x 32-bit arithmetic, independent of the product path).

This build runs the dense rounds only: the optimised partial rounds of the plan are not built, so the
tests of their self-check do not exist; test_round_plan_switch_is_accepted_and_dense pins what the switch does meanwhile."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import blaze_amd
import poseidon_fixtures
import poseidon_ref as R
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd._lib import buf_ptr, check
from blaze_amd.driver_client import DriverClient
from blaze_amd.ingo_hash import (Hash, PoseidonClient, PoseidonImageParametrs, PoseidonInitializeParameters, PoseidonResult, TreeMode,
                                 num_of_elements_in_base_layer)

pytestmark = pytest.mark.gpu

FIXTURE = poseidon_fixtures.path("bls381_t9_t12")
SMALL = {f: poseidon_fixtures.path(f"{f.lower()}_small") for f in R.FIELD_ID}
TEST_SCALAR = 15338226384362629345253584946022322145063321004547266825580649561525819500264   # integration_poseidon.rs:24-25

_words, _blocks, _trees = {}, {}, {}


def words_of(path):
    if path not in _words:
        _words[path] = R.read_instruction_words(path)
        _blocks[path] = R.parse_stream(_words[path])[0]
    return _words[path]


def blocks_of(path):
    words_of(path)
    return _blocks[path]


def params_for(field, big=False):
    return FIXTURE if (field == "BLS381" and big) else SMALL[field]


def elements(n, r, seed):
    rng = random.Random(seed)
    return [rng.randrange(r) for _ in range(n)]


def el_bytes(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def n_inputs(h, mode):
    return (11 if mode == TreeMode.TreeC else 1) * 8 ** (h - 1)


def py_tree(field, path, h, mode, seed):
    """(elements, {(layer, id): digest}) - cached: the h = 5 tree costs 15 s of Python"""
    key = (field, path, h, int(mode), seed)
    if key not in _trees:
        r = R.MODULUS[field]
        el = elements(n_inputs(h, mode), r, seed)
        _trees[key] = (el, R.tree(el, h, int(mode), blocks_of(path), r))
    return _trees[key]


def client(gpu, field="BLS381"):
    return PoseidonClient(Hash.Poseidon, DriverClient(0), field=field)


def as_dict(results):
    out = {}
    for x in results:
        key = (x.layer_id, x.hash_id)
        assert key not in out, f"record {key} twice"
        out[key] = int.from_bytes(x.hash_byte, "little")
    return out


def assert_children_first(results):
    seen = set()
    for x in results:
        if x.layer_id > 0:
            for k in range(8):
                child = (x.layer_id - 1, 8 * x.hash_id + k)
                assert child in seen or child[0] < first_layer_of(results), f"parent {(x.layer_id, x.hash_id)} before its child {child}"
        seen.add((x.layer_id, x.hash_id))


def first_layer_of(results):
    return min(x.layer_id for x in results)


# ---------------------------------------------------------------------------------------------- 5. the permutation

@pytest.mark.parametrize("field,t,big", [(f, t, False) for f in ("BLS377", "BLS381", "BN254") for t in (3, 9, 12)] +
                         [("BLS381", 9, True), ("BLS381", 12, True)])
def test_definition_kernel_equals_python(gpu, field, t, big):
    """4096 random states through the definition kernel, bit for bit (the fixture's (8, 57) rounds on BLS12-381 too)"""
    path = params_for(field, big)
    r = R.MODULUS[field]
    wb = R.words_bytes(words_of(path))
    n = 4096
    rng = random.Random(1000 * t + len(field))
    states = [[rng.randrange(r) for _ in range(t)] for _ in range(n)]
    states[0] = [0] * t
    states[1] = [r - 1] * t
    raw = bytearray(el_bytes([x for s in states for x in s]))
    out = bytearray(len(raw))
    check(blaze_amd.aux().blz_test_poseidon_permute(0, R.FIELD_ID[field], buf_ptr(wb)[0], len(wb), t, buf_ptr(raw)[0], buf_ptr(out)[0], n))
    blk = blocks_of(path)[t]
    for i, s in enumerate(states):
        want = el_bytes(R.permute(s, blk, r))
        assert bytes(out[i * t * 32:(i + 1) * t * 32]) == want, f"state {i}"


@pytest.mark.parametrize("field,t,big", [(f, t, False) for f in ("BLS377", "BLS381", "BN254") for t in (3, 9, 12)] +
                         [("BLS381", 9, True), ("BLS381", 12, True)])
def test_product_path_equals_definition_kernel(gpu, field, t, big):
    """2^16 inputs per width through the tree's kernel and through the definition kernel: equal digests.  Inputs: random field
    elements, all-zero, all r - 1, and words that are not canonical (r, r + 1, 2^256 - 1, random 256-bit words)."""
    path = params_for(field, big)
    r = R.MODULUS[field]
    wb = R.words_bytes(words_of(path))
    blk = blocks_of(path)[t]
    n, a = 1 << 16, t - 1
    rs = np.random.RandomState(77 * t + len(field))
    inp = rs.randint(0, 256, size=(n, a, 32), dtype=np.uint8)
    inp[:, :, 31] &= (1 << (r.bit_length() - 1 - 248)) - 1          # < 2^(bits - 1) < r: canonical
    special = {0: 0, 1: r - 1, 2: r, 3: r + 1, 4: (1 << 256) - 1}
    for row, v in special.items():
        inp[row] = np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)
    inp[5:2048] = rs.randint(0, 256, size=(2043, a, 32), dtype=np.uint8)          # any 256-bit words
    inp = np.ascontiguousarray(inp)
    dig = np.zeros((n, 32), dtype=np.uint8)
    check(blaze_amd.aux().blz_test_poseidon_hash(0, R.FIELD_ID[field], buf_ptr(wb)[0], len(wb), t, buf_ptr(inp)[0], buf_ptr(dig)[0], n))
    states = np.zeros((n, t, 32), dtype=np.uint8)
    states[:, 0] = np.frombuffer(int(blk["tag"]).to_bytes(32, "little"), dtype=np.uint8)
    states[:, 1:] = inp
    states = np.ascontiguousarray(states)
    out = np.zeros_like(states)
    check(blaze_amd.aux().blz_test_poseidon_permute(0, R.FIELD_ID[field], buf_ptr(wb)[0], len(wb), t, buf_ptr(states)[0], buf_ptr(out)[0], n))
    bad = np.nonzero((out[:, 1] != dig).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} digests differ, first at input {bad[:5]}"
    # ... and both are the Python hash (the special rows and a few random ones)
    for row in list(special) + [5, 100, 2047, 2048, n - 1]:
        vals = [int.from_bytes(inp[row, k].tobytes(), "little") for k in range(a)]
        assert int.from_bytes(dig[row].tobytes(), "little") == R.hash_fixed(vals, blk, r), row


def _product_against_definition(field, wb, blk, t, n, seed):
    """n random inputs (a few of them not canonical) through the tree's kernel and through the definition kernel; a few rows by Python"""
    r = R.MODULUS[field]
    a = t - 1
    rs = np.random.RandomState(seed)
    inp = rs.randint(0, 256, size=(n, a, 32), dtype=np.uint8)
    inp[16:, :, 31] &= (1 << (r.bit_length() - 1 - 248)) - 1          # rows 0 .. 15: any 256-bit words
    inp = np.ascontiguousarray(inp)
    dig = np.zeros((n, 32), dtype=np.uint8)
    check(blaze_amd.aux().blz_test_poseidon_hash(0, R.FIELD_ID[field], buf_ptr(wb)[0], len(wb), t, buf_ptr(inp)[0], buf_ptr(dig)[0], n))
    states = np.zeros((n, t, 32), dtype=np.uint8)
    states[:, 0] = np.frombuffer(int(blk["tag"]).to_bytes(32, "little"), dtype=np.uint8)
    states[:, 1:] = inp
    states = np.ascontiguousarray(states)
    out = np.zeros_like(states)
    check(blaze_amd.aux().blz_test_poseidon_permute(0, R.FIELD_ID[field], buf_ptr(wb)[0], len(wb), t, buf_ptr(states)[0], buf_ptr(out)[0], n))
    bad = np.nonzero((out[:, 1] != dig).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} digests differ, first at input {bad[:5]}"
    for row in (0, 1, 16, 17, n - 1):
        st = [int.from_bytes(states[row, k].tobytes(), "little") for k in range(t)]
        assert b"".join(out[row, k].tobytes() for k in range(t)) == el_bytes(R.permute(st, blk, r)), row     # the whole state, not state[1] alone
        assert int.from_bytes(dig[row].tobytes(), "little") == R.hash_fixed(st[1:], blk, r), row


@pytest.mark.parametrize("field", ["BLS377", "BLS381", "BN254"])
def test_matrix_that_is_not_symmetric(gpu, field):
    """The tool's Cauchy matrices are symmetric: a kernel that multiplied by the TRANSPOSE would pass every other test.  Here every
    block's matrix is random: the definition kernel, the product path and a small tree against Python's row-major sum."""
    r = R.MODULUS[field]
    words = poseidon_fixtures.with_random_matrices(words_of(SMALL[field]), r, 21)
    blocks = R.parse_stream(words)[0]
    wb = R.words_bytes(words)
    for t in (3, 9, 12):
        assert any(blocks[t]["mds"][i][j] != blocks[t]["mds"][j][i] for i in range(t) for j in range(i))
        _product_against_definition(field, wb, blocks[t], t, 4096, 5 * t)
    for mode, h in ((TreeMode.TreeC, 2), (TreeMode.TreeD, 3)):
        el = elements(n_inputs(h, mode), r, 31)
        cl = client(gpu, field)
        cl.initialize_words(h, mode, wb)
        run_tree(cl, el)
        assert as_dict(cl.result(R.num_records(h, int(mode)))) == R.tree(el, h, int(mode), blocks, r)
        cl.close()


@pytest.mark.parametrize("field", ["BLS381", "BN254"])
def test_every_shape_of_row_product_runs(gpu, field):
    """widths the trees never use: one, two and three reductions per matrix row, full and partial last groups (t = 2, 6, 7, 13, 16; also 4
    and 15), on a generated stream with random matrices"""
    r = R.MODULUS[field]
    widths = (2, 4, 6, 7, 13, 15, 16)
    words = poseidon_fixtures.with_random_matrices(poseidon_fixtures.tool().generate(field, [(t, 8, 5) for t in widths]), r, 41)
    blocks = R.parse_stream(words)[0]
    wb = R.words_bytes(words)
    for t in widths:
        _product_against_definition(field, wb, blocks[t], t, 2048, 7 * t)


# ---------------------------------------------------------------------------------------------- 6. trees against Python

def run_tree(cl, el, chunks=None):
    data = el_bytes(el)
    if chunks is None:
        cl.set_data(data)
    else:
        pos = 0
        k = 0
        while pos < len(el):
            c = chunks[k % len(chunks)]
            cl.set_data(data[32 * pos: 32 * (pos + c)])
            pos += c
            k += 1


@pytest.mark.parametrize("mode,h", [(TreeMode.TreeC, h) for h in (1, 2, 3, 4, 5)] + [(TreeMode.TreeD, h) for h in (2, 3, 4, 5)])
def test_trees_on_bls381_equal_python_record_by_record(gpu, mode, h):
    el, want = py_tree("BLS381", FIXTURE, h, mode, 5)
    cl = client(gpu)
    cl.initialize(PoseidonInitializeParameters(h, mode, FIXTURE))
    run_tree(cl, el)
    n = R.num_records(h, int(mode))
    res = cl.result(n)
    assert len(res) == n and cl.get_num_of_pending_results() == 0
    assert as_dict(res) == want
    assert_children_first(res)
    cl.close()


@pytest.mark.parametrize("field", ["BLS377", "BN254"])
@pytest.mark.parametrize("mode,h", [(TreeMode.TreeC, 1), (TreeMode.TreeC, 2), (TreeMode.TreeC, 3), (TreeMode.TreeD, 2), (TreeMode.TreeD, 3)])
def test_trees_on_the_other_fields(gpu, field, mode, h):
    el, want = py_tree(field, SMALL[field], h, mode, 6)
    cl = client(gpu, field)
    cl.initialize_words(h, mode, R.words_bytes(words_of(SMALL[field])))
    run_tree(cl, el)
    res = cl.result(R.num_records(h, int(mode)))
    assert as_dict(res) == want
    cl.close()


def test_build_small_tree(gpu):
    """integration_poseidon.rs:122-169: height 4, 5632 calls of one element (TEST_SCALAR.to_bytes_le()), result(585) - and every
    digest checked, which the reference never does"""
    cl = client(gpu)
    params = PoseidonInitializeParameters(4, TreeMode.TreeC, FIXTURE)
    nof_elements = num_of_elements_in_base_layer(params.tree_height)
    cl.log_api_values()
    cl.initialize(params)
    ib = cl.loaded_binary_parameters()
    assert len(ib) == 2
    m = PoseidonImageParametrs.parse_image_params(ib[1])
    assert m.hif2_cpu_c_is_stub == 0 and m.hif2_cpu_c_number_of_cores >= 1 and m.hif2_cpu_c_place_holder == 0
    scalar = TEST_SCALAR.to_bytes((TEST_SCALAR.bit_length() + 7) // 8, "little")
    for _ in range(nof_elements):
        for _ in range(11):
            cl.set_data(scalar)
    result = cl.result(585)
    assert len(result) == 585
    want = R.tree([TEST_SCALAR] * (11 * 512), 4, R.TREE_C, blocks_of(FIXTURE), R.MODULUS["BLS381"])
    assert as_dict(result) == want
    assert_children_first(result)
    assert cl.get_last_hash_sent_to_host() == result[-1].hash_id
    cl.close()


def test_sanity_check(gpu):
    """integration_poseidon.rs:29-57: height 8, 4-byte writes, the element counter goes up by exactly one per call"""
    cl = client(gpu)
    cl.initialize(PoseidonInitializeParameters(8, TreeMode.TreeC, FIXTURE))
    cl.set_data((0).to_bytes(4, "little"))
    f = cl.get_last_element_sent_to_ring()
    cl.set_data((1).to_bytes(4, "little"))
    n = cl.get_last_element_sent_to_ring()
    assert f != n and n == f + 1
    assert cl.info()["device_bytes"] >= 11 * 8 ** 7 * 32
    cl.close()


# ---------------------------------------------------------------------------------------------- 7. feeding does not change bytes

def test_feeding_does_not_change_bytes(gpu):
    h, mode = 5, TreeMode.TreeC
    el, want = py_tree("BLS381", FIXTURE, h, mode, 5)
    n = R.num_records(h, int(mode))
    cl = client(gpu)
    cl.initialize(PoseidonInitializeParameters(h, mode, FIXTURE))
    # 2048-element slices, polling like the reference's threaded test (integration_poseidon.rs:87-99)
    got, data = [], el_bytes(el)
    for pos in range(0, len(el), 2048):
        cl.set_data(data[32 * pos: 32 * (pos + 2048)])
        got += PoseidonResult.parse_poseidon_hash_results(cl.get_raw_results(cl.get_num_of_pending_results()))
    got += cl.result(n - len(got))
    assert as_dict(got) == want
    assert_children_first(got)
    # ragged slices that straddle node (11) and column boundaries
    run_tree(cl, el, chunks=[1, 10, 12, 7, 350, 4097, 3, 11 * 8 * 8 + 5, 2])
    got = []
    while len(got) < n:
        part = cl.result(1000)
        assert part, "no more records"
        got += part
    assert as_dict(got) == want
    assert_children_first(got)
    # from a DeviceBuffer, read back through tree_device: (layer, id) order
    d_in = DeviceBuffer(0, len(data))
    d_in.upload(data)
    cl.set_data(d_in)
    cl.wait_result()
    assert cl.get_num_of_pending_results() == n
    d_out = DeviceBuffer(0, 64 * n)
    cl.tree_device(d_out)
    assert cl.get_num_of_pending_results() == 0
    rec = PoseidonResult.parse_poseidon_hash_results(d_out.download())
    assert [(x.layer_id, x.hash_id) for x in rec] == sorted(want)
    assert as_dict(rec) == want
    with pytest.raises(DriverClientError):
        cl.tree_device(d_out)                       # popped: nothing left to hand over
    ms = cl.last_kernel_ms()
    assert 0 < ms < 10_000
    d_in.free()
    d_out.free()
    cl.close()


def test_element_by_element_back_to_back_trees_and_reset(gpu):
    h, mode = 3, TreeMode.TreeC
    el, want = py_tree("BLS381", FIXTURE, h, mode, 8)
    el2, want2 = py_tree("BLS381", FIXTURE, h, mode, 9)
    n = R.num_records(h, int(mode))
    cl = client(gpu)
    cl.initialize(PoseidonInitializeParameters(h, mode, FIXTURE))
    for i, v in enumerate(el):
        cl.set_data(int(v).to_bytes(32, "little"))
        assert cl.get_last_element_sent_to_ring() == i + 1
    assert cl.get_num_of_pending_results() == n
    # a second tree right behind the first, in one call together with the first element of a third: the ids restart, the first
    # tree's unread records stay pending
    cl.set_data(el_bytes(el2 + el[:1]))
    assert cl.get_num_of_pending_results() == 2 * n
    # ... a third tree completes and a fourth begins while the records of the first two are still unread
    cl.set_data(el_bytes(el[1:] + el2[:1]))
    assert cl.get_num_of_pending_results() == 3 * n
    with pytest.raises(DriverClientError):
        cl.tree_device(DeviceBuffer(0, 64 * n))      # older records are pending: nothing to hand over as "the tree"
    first = cl.result(n)
    second = cl.result(n)
    third = PoseidonResult.parse_poseidon_hash_results(cl.get_raw_results(n))
    assert as_dict(first) == want and as_dict(second) == want2 and as_dict(third) == want
    assert cl.get_num_of_pending_results() == 0
    # reset mid-tree drops the partial tree (one element so far) and nothing else: the next elements are a whole new tree
    cl.set_data(el_bytes(el[1:200]))
    cl.reset()
    assert cl.get_num_of_pending_results() == 0
    assert cl.result(5) == []
    run_tree(cl, el2)
    assert as_dict(cl.result(n)) == want2
    cl.close()


# ---------------------------------------------------------------------------------------------- 8. large trees

@pytest.mark.parametrize("h", [7, 8])
def test_large_tree_every_node_through_the_definition_kernel(gpu, h):
    """TreeC with 2^18 / 2^21 columns from synthetic device inputs: EVERY node re-hashed from its children by the definition kernel
    and compared on the device; 64 sampled nodes per layer and the whole top three layers by Python on top of that."""
    mode = TreeMode.TreeC
    r = R.MODULUS["BLS381"]
    blocks = blocks_of(FIXTURE)
    wb = R.words_bytes(words_of(FIXTURE))
    n_in, n_rec = n_inputs(h, mode), R.num_records(h, int(mode))
    d_in = DeviceBuffer(0, 32 * n_in)
    check(blaze_amd.aux().blz_synth_field_elements(0, d_in.ptr, n_in, 4242 + h))
    cl = client(gpu)
    cl.initialize(PoseidonInitializeParameters(h, mode, FIXTURE))
    cl.set_data(d_in)
    cl.wait_result()
    print(f"TreeC h = {h}: {cl.last_kernel_ms():.2f} ms for {n_rec} hashes")
    d_rec = DeviceBuffer(0, 64 * n_rec)
    cl.tree_device(d_rec)
    out = (C.c_uint64 * 2)()
    check(blaze_amd.aux().blz_test_poseidon_tree_check(0, 1, buf_ptr(wb)[0], len(wb), int(mode), h, d_in.ptr, d_rec.ptr, out))
    assert out[0] == n_rec, f"only {out[0]} of {n_rec} nodes went through the definition kernel"
    assert out[1] == 0, f"{out[1]} nodes differ from the definition kernel"
    # the supplement: Python on samples
    off = {}
    pos = 0
    for layer in range(h):
        off[layer] = pos
        pos += 8 ** (h - 1 - layer)
    rng = random.Random(h)

    def record(layer, i):
        x = PoseidonResult.parse_poseidon_hash_results(d_rec.download(64, 64 * (off[layer] + i)))[0]
        assert (x.layer_id, x.hash_id) == (layer, i)
        return int.from_bytes(x.hash_byte, "little")

    for layer in range(h):
        count = 8 ** (h - 1 - layer)
        ids = range(count) if layer >= h - 3 else sorted(rng.sample(range(count), 64))
        for i in ids:
            if layer == 0:
                raw = d_in.download(11 * 32, 11 * 32 * i)
                kids = [int.from_bytes(raw[32 * k: 32 * k + 32], "little") for k in range(11)]
                want = R.hash_fixed(kids, blocks[12], r)
            else:
                raw = d_rec.download(8 * 64, 64 * (off[layer - 1] + 8 * i))
                kids = [int.from_bytes(raw[64 * k: 64 * k + 32], "little") for k in range(8)]
                want = R.hash_fixed(kids, blocks[9], r)
            assert record(layer, i) == want, (layer, i)
    d_in.free()
    d_rec.free()
    cl.close()


# ---------------------------------------------------------------------------------------------- 9. / 10. switches, waits, errors

def test_round_plan_switch_is_accepted_and_dense(gpu):
    """the optimised partial rounds are not built: info says so, both settings of the switch give the same (dense) records"""
    h, mode = 3, TreeMode.TreeD
    el, want = py_tree("BLS381", FIXTURE, h, mode, 11)
    cl = client(gpu)
    cl.initialize(PoseidonInitializeParameters(h, mode, FIXTURE))
    info = cl.info()
    assert info["optimised_partial_rounds"] is False and info["round_plan_check"] == 0 and info["width_mask"] == (1 << 9) | (1 << 12)
    for enable in (False, True):
        cl.set_round_plan(enable)
        run_tree(cl, el)
        assert as_dict(cl.result(R.num_records(h, int(mode)))) == want
    assert blaze_amd.lib().blz_poseidon_set_round_plan(cl._h, 2) == 4
    cl.close()


def test_bounded_result_and_refusals_change_nothing(gpu, tmp_path):
    import time

    L = blaze_amd.lib()
    cl = client(gpu)
    one = (7).to_bytes(32, "little")
    with pytest.raises(DriverClientError) as ei:
        cl.set_data(one)                                        # before initialize
    assert ei.value.variant == "InvalidPrimitiveParam"
    with pytest.raises(DriverClientError) as ei:
        cl.wait_result()
    assert ei.value.variant == "InvalidPrimitiveParam"
    with pytest.raises(DriverClientError) as ei:
        cl.initialize(PoseidonInitializeParameters(12, TreeMode.TreeC, FIXTURE))    # hash_id would not fit 30 bits
    assert ei.value.variant == "InvalidPrimitiveParam"
    with pytest.raises(DriverClientError) as ei:
        cl.initialize(PoseidonInitializeParameters(11, TreeMode.TreeC, FIXTURE))    # 378 GB of input: does not fit the device
    assert ei.value.variant == "InvalidPrimitiveParam"
    assert cl.info()["width_mask"] == 0 and cl.info()["device_bytes"] == 0

    # load failures: LoadFailed, and the handle stays what it was - here: uninitialised
    words = words_of(FIXTURE)
    r = R.MODULUS["BLS381"]

    def edit(i, v):
        w = list(words)
        w[i] = v
        return R.words_bytes(w)

    bad_streams = [R.words_bytes(words[:-40]), edit(100, r), edit(4, 3), edit(5, 7), edit(3, 17), edit(0, 12345),
                   R.words_bytes([words[0], words[1], 1] + words[3 + 5 + 9 * 65 + 81:1603])]
    for wb in bad_streams:
        with pytest.raises(DriverClientError) as ei:
            cl.initialize_words(2, TreeMode.TreeC, wb)
        assert ei.value.variant == "LoadFailed", ei.value
    with pytest.raises(DriverClientError) as ei:
        cl.initialize(PoseidonInitializeParameters(2, TreeMode.TreeC, str(tmp_path / "missing.csv")))
    assert ei.value.variant == "LoadFailed" and "missing.csv" in str(ei.value)
    bad_csv = tmp_path / "bad.csv"
    bad_csv.write_text(open(FIXTURE).read().replace(",5\n", ",3\n", 1))             # alpha = 3 in the first block
    with pytest.raises(DriverClientError) as ei:
        cl.initialize(PoseidonInitializeParameters(2, TreeMode.TreeC, str(bad_csv)))
    assert ei.value.variant == "LoadFailed" and "bad.csv" in str(ei.value)
    assert cl.info()["width_mask"] == 0
    with pytest.raises(DriverClientError):
        cl.set_data(one)

    # ... and an initialised handle keeps its tree through the same failures
    h, mode = 2, TreeMode.TreeC
    el, want = py_tree("BLS381", FIXTURE, h, mode, 12)
    cl.initialize(PoseidonInitializeParameters(h, mode, FIXTURE))
    run_tree(cl, el[:50])
    before = (cl.info(), cl._counters(), cl.get_num_of_pending_results())
    for wb in bad_streams[:3]:
        with pytest.raises(DriverClientError):
            cl.initialize_words(3, TreeMode.TreeD, wb)
    with pytest.raises(DriverClientError):
        cl.initialize(PoseidonInitializeParameters(3, TreeMode.TreeC, str(tmp_path / "missing.csv")))
    with pytest.raises(DriverClientError) as ei:
        cl.set_data(bytes(33))                                  # neither whole elements nor one short element
    assert ei.value.variant == "InvalidPrimitiveParam"
    with pytest.raises(DriverClientError):
        cl.initialize(PoseidonInitializeParameters(12, mode, FIXTURE))
    assert L.blz_poseidon_raw_results(cl._h, 1, buf_ptr(bytearray(64))[0], 64) == 4     # nothing pending yet
    assert (cl.info(), cl._counters(), cl.get_num_of_pending_results()) == before

    # result(expected) beyond what the fed elements can produce: short, not late.  50 elements = 4 complete base nodes
    t0 = time.time()
    part = cl.result(9)
    assert time.time() - t0 < 5.0
    assert sorted((x.layer_id, x.hash_id) for x in part) == [(0, 0), (0, 1), (0, 2), (0, 3)]
    assert all(int.from_bytes(x.hash_byte, "little") == want[(0, x.hash_id)] for x in part)
    assert cl.result(9) == []
    run_tree(cl, el[50:])
    rest = cl.result(9)
    assert as_dict(part + rest) == want
    cl.close()
