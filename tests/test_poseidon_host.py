"""The Poseidon tree client, the part that needs no device: the C ABI and its Python mirror, the load-time checks of the instruction
word stream (blz_poseidon_check_words), the parameter tool's output (pinned by digest under tests/golden/), and the 64-byte record
against a transcription of the reference's parser."""
import ctypes as C
import os
import re

import pytest

import blaze_amd
import poseidon_fixtures
import poseidon_ref as R
from blaze_amd import DriverClientError
from blaze_amd._lib import AUX_EXPORTED_SYMBOLS, EXPORTED_SYMBOLS
from blaze_amd.driver_client import DriverPrimitive
from blaze_amd.ingo_hash import (Hash, PoseidonClient, PoseidonImageParametrs, PoseidonInitializeParameters, PoseidonResult, TreeMode,
                                 check_words, num_of_elements_in_base_layer, num_of_elements_oct_tree)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = poseidon_fixtures.path("bls381_t9_t12")
SMALL = {f: poseidon_fixtures.path(f"{f.lower()}_small") for f in R.FIELD_ID}

FUNCTIONS = ("new", "free", "loaded_binary_parameters", "initialize", "check_words", "initialize_words", "set_data", "set_data_device",
             "wait_result", "num_pending_results", "raw_results", "result", "tree_device", "counters", "info", "set_round_plan",
             "last_kernel_ms", "stream", "reset")


def _ptr(b):
    return C.cast(C.c_char_p(b), C.c_void_p)


def test_entry_points_in_every_layer():
    hdr = open(os.path.join(ROOT, "include", "blaze_hip.h")).read()
    raw = C.CDLL(blaze_amd._lib.LIB_PATH)
    for f in FUNCTIONS:
        name = "blz_poseidon_" + f
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in EXPORTED_SYMBOLS and getattr(raw, name) is not None
    assert re.search(r"enum\s+blz_tree_mode\s*\{\s*BLZ_TREE_C\s*=\s*0\s*,\s*BLZ_TREE_D\s*=\s*1\s*\}", hdr)
    for name in ("blz_test_poseidon_permute", "blz_test_poseidon_hash", "blz_test_poseidon_tree_check"):
        assert name in AUX_EXPORTED_SYMBOLS and getattr(blaze_amd.aux(), name) is not None


def test_python_mirror_follows_the_reference():
    assert issubclass(PoseidonClient, DriverPrimitive) and not getattr(PoseidonClient, "__abstractmethods__", None)
    assert [m.name for m in TreeMode] == ["TreeC", "TreeD"] and [int(m) for m in TreeMode] == [0, 1]      # utils.rs:18-30
    assert Hash.Poseidon is not None
    import dataclasses
    assert [f.name for f in dataclasses.fields(PoseidonInitializeParameters)] == ["tree_height", "tree_mode", "instruction_path"]
    assert [f.name for f in dataclasses.fields(PoseidonResult)] == ["hash_byte", "hash_id", "layer_id"]
    for m in ("get_num_of_pending_results", "get_raw_results", "get_last_element_sent_to_ring", "get_last_hash_sent_to_host", "log_api_values"):
        assert callable(getattr(PoseidonClient, m))
    with pytest.raises(NotImplementedError):
        PoseidonClient.start_process(object())                                   # todo!() in the reference
    assert num_of_elements_oct_tree(4) == 585 and num_of_elements_in_base_layer(4) == 512      # integration_poseidon.rs:23
    assert [R.num_records(h, R.TREE_C) for h in (1, 2, 4)] == [1, 9, 585] and R.num_records(4, R.TREE_D) == 73


def test_arguments_are_checked_before_any_device_is_touched():
    L = blaze_amd.lib()
    h = C.c_void_p()
    assert L.blz_poseidon_new(0, 7, C.byref(h)) == 4 and not h.value       # unknown field
    assert L.blz_poseidon_new(0, 1, None) == 4
    buf = (C.c_uint8 * 64)()
    n32 = C.c_uint32()
    u32x4 = (C.c_uint32 * 4)()
    u64x4 = (C.c_uint64 * 4)()
    fl = C.c_float()
    assert L.blz_poseidon_loaded_binary_parameters(None, u32x4) == 4
    assert L.blz_poseidon_initialize(None, 4, 0, b"x.csv") == 4
    assert L.blz_poseidon_initialize_words(None, 4, 0, C.cast(buf, C.c_void_p), 64) == 4
    assert L.blz_poseidon_set_data(None, C.cast(buf, C.c_void_p), 32) == 4
    assert L.blz_poseidon_set_data_device(None, None, 32) == 4
    assert L.blz_poseidon_wait_result(None) == 4
    assert L.blz_poseidon_num_pending_results(None, C.byref(n32)) == 4
    assert L.blz_poseidon_raw_results(None, 1, C.cast(buf, C.c_void_p), 64) == 4
    assert L.blz_poseidon_result(None, 1, C.cast(buf, C.c_void_p), 64, C.byref(n32)) == 4
    assert L.blz_poseidon_tree_device(None, None, 0) == 4
    assert L.blz_poseidon_counters(None, u32x4) == 4
    assert L.blz_poseidon_info(None, u64x4) == 4
    assert L.blz_poseidon_set_round_plan(None, 1) == 4
    assert L.blz_poseidon_last_kernel_ms(None, C.byref(fl)) == 4
    assert L.blz_poseidon_stream(None, None, None) == 4
    assert L.blz_poseidon_reset(None) == 4
    L.blz_poseidon_free(None)
    wb = R.words_bytes(R.read_instruction_words(FIXTURE))
    assert L.blz_poseidon_check_words(9, 0, _ptr(wb), len(wb), u32x4) == 4    # unknown field
    assert L.blz_poseidon_check_words(1, 2, _ptr(wb), len(wb), u32x4) == 4    # unknown tree mode
    assert L.blz_poseidon_check_words(1, 0, None, 0, u32x4) == 4


@pytest.mark.skipif(blaze_amd.lib().blz_device_count() > 0, reason="a GPU is present")
def test_no_gpu_means_file_error():
    L = blaze_amd.lib()
    h = C.c_void_p()
    assert L.blz_poseidon_new(0, 1, C.byref(h)) == 7 and not h.value
    assert b"no CPU path" in L.blz_last_error_message()


def test_parameter_files_are_the_pinned_bytes():
    """the tool writes, byte for byte, what tests/golden/poseidon_params.json pins (the CSVs themselves are too large to commit)"""
    import hashlib
    assert set(poseidon_fixtures.PINNED) == {"bls381_t9_t12", "bls377_small", "bls381_small", "bn254_small"}
    assert poseidon_fixtures.PINNED["bls381_t9_t12"]["blocks"] == [[9, 8, 57], [12, 8, 57]]
    for name, spec in poseidon_fixtures.PINNED.items():
        text = poseidon_fixtures.generate(name)
        assert len(text) == spec["bytes"] and hashlib.sha256(text).hexdigest() == spec["sha256"], name
        assert open(poseidon_fixtures.path(name), "rb").read() == text
    # ... and the command line writes the same bytes
    import subprocess
    import sys
    cli = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "poseidon_params.py"), "--field", "BN254", "--block", "3,8,5", "--block", "9,8,5",
                          "--block", "12,8,5"], check=True, capture_output=True).stdout
    assert cli == poseidon_fixtures.generate("bn254_small")


def _rank(m, r):
    a = [[x % r for x in row] for row in m]
    rank = 0
    for c in range(len(a[0])):
        p = next((k for k in range(rank, len(a)) if a[k][c]), None)
        if p is None:
            continue
        a[rank], a[p] = a[p], a[rank]
        inv = pow(a[rank][c], -1, r)
        a[rank] = [x * inv % r for x in a[rank]]
        for k in range(len(a)):
            if k != rank and a[k][c]:
                f = a[k][c]
                a[k] = [(x - f * y) % r for x, y in zip(a[k], a[rank])]
        rank += 1
    return rank


@pytest.mark.parametrize("field,path", [("BLS381", FIXTURE)] + sorted(SMALL.items()), ids=["BLS381-t9-t12", "BLS377-small", "BLS381-small", "BN254-small"])
def test_fixture_matrices_hold_what_the_tool_claims(field, path):
    """every block: words below r, tag_t = 2^(t-1) - 1, M the Cauchy matrix 1 / (i + t + j), M invertible, and M without row 0 and
    column 0 invertible (re-checked here with this file's own elimination)"""
    r = R.MODULUS[field]
    words = R.read_instruction_words(path)
    assert all(0 <= w < r for w in words) and len(words) % 2 == 0
    blocks, fid = R.parse_stream(words)
    assert fid == R.FIELD_ID[field] and {9, 12} <= set(blocks)
    for t, b in blocks.items():
        assert b["tag"] == (1 << (t - 1)) - 1 and b["rf"] % 2 == 0 and len(b["rc"]) == b["rf"] + b["rp"]
        for i in range(t):
            for j in range(t):
                assert b["mds"][i][j] * (i + t + j) % r == 1
        assert _rank(b["mds"], r) == t
        assert _rank([row[1:] for row in b["mds"][1:]], r) == t - 1
        flat = [c for rnd in b["rc"] for c in rnd]
        assert len(set(flat)) == len(flat)          # (a stuck generator would repeat)


def test_check_words_accepts_the_fixture():
    words = R.read_instruction_words(FIXTURE)
    assert len(words) == 1604 and words[-1] == 0       # 1603 words and the pad
    wb = R.words_bytes(words)
    assert check_words("BLS381", TreeMode.TreeC, wb) == {"blocks": 2, "width_mask": (1 << 9) | (1 << 12), "optimised_partial_rounds": False, "words": 1603}
    assert check_words("BLS381", TreeMode.TreeD, wb)["blocks"] == 2
    assert check_words("BLS381", TreeMode.TreeC, wb[:-32])["words"] == 1603     # the pad is optional in memory
    for f, path in SMALL.items():
        got = check_words(f, TreeMode.TreeC, R.words_bytes(R.read_instruction_words(path)))
        assert got["blocks"] == 3 and got["width_mask"] == (1 << 3) | (1 << 9) | (1 << 12)


def _refused(field, mode, words):
    with pytest.raises(DriverClientError) as ei:
        check_words(field, mode, R.words_bytes(words) if isinstance(words, list) else words)
    assert ei.value.variant == "LoadFailed", ei.value
    return str(ei.value)


def test_check_words_refuses_what_the_header_says_it_refuses():
    r = R.MODULUS["BLS381"]
    words = R.read_instruction_words(FIXTURE)
    blocks, _ = R.parse_stream(words)
    t9 = 3                                     # word index of the first block's header (t, alpha, R_F, R_P, tag)
    assert words[t9:t9 + 4] == [9, 5, 8, 57]
    t12 = t9 + 5 + 9 * 65 + 81
    assert words[t12:t12 + 4] == [12, 5, 8, 57]

    def edit(i, v):
        w = list(words)
        w[i] = v
        return w

    assert "truncated" in _refused("BLS381", TreeMode.TreeC, words[:-40])                     # truncated block
    assert "truncated" in _refused("BLS381", TreeMode.TreeC, words[:5])
    assert "not a whole number" in _refused("BLS381", TreeMode.TreeC, R.words_bytes(words)[:-7])
    assert "modulus" in _refused("BLS381", TreeMode.TreeC, edit(100, r))                      # word >= r
    assert "modulus" in _refused("BLS381", TreeMode.TreeC, edit(1500, (1 << 256) - 1))
    assert "alpha" in _refused("BLS381", TreeMode.TreeC, edit(t9 + 1, 3))                     # alpha != 5
    assert "R_F" in _refused("BLS381", TreeMode.TreeC, edit(t9 + 2, 7))                       # odd R_F
    assert "width out of range" in _refused("BLS381", TreeMode.TreeC, edit(t9, 17))           # t out of range
    assert "width out of range" in _refused("BLS381", TreeMode.TreeC, edit(t9, 1))
    assert "magic" in _refused("BLS381", TreeMode.TreeC, edit(0, words[0] + 1))               # wrong magic
    assert "magic" in _refused("BLS381", TreeMode.TreeC, [1, 2, 3, 4, 5, 6])                  # (a CSV made for something else)
    assert "another field" in _refused("BN254", TreeMode.TreeC, [w % R.MODULUS["BN254"] for w in words])
    assert "twice" in _refused("BLS381", TreeMode.TreeC, edit(t12, 9))
    assert "pad" in _refused("BLS381", TreeMode.TreeC, edit(len(words) - 1, 1))
    assert "follow the last block" in _refused("BLS381", TreeMode.TreeC, words + [0, 0])
    # a width the tree mode needs is missing: the t = 9 block alone serves TreeD, not TreeC
    only9 = [words[0], words[1], 1] + words[t9:t12]
    only9 += [0] * (len(only9) % 2)
    assert check_words("BLS381", TreeMode.TreeD, R.words_bytes(only9))["width_mask"] == 1 << 9
    assert "missing" in _refused("BLS381", TreeMode.TreeC, only9)
    only12 = [words[0], words[1], 1] + words[t12:1603]
    only12 += [0] * (len(only12) % 2)
    assert "missing" in _refused("BLS381", TreeMode.TreeD, only12)
    assert blocks[9]["rp"] == 57


def test_record_packing_against_the_reference_parser():
    for layer in range(11):
        for hid in (0, 1, (1 << 30) - 1):
            digest = (0x1234567890ABCDEF << 180) | (layer << 8) | (hid & 0xFF)
            rec = R.pack_record(digest, hid, layer)
            assert len(rec) == 64 and rec[37:] == bytes(27)
            assert R.parse_poseidon_hash_results(rec) == [(digest.to_bytes(32, "little"), hid, layer)]
            got = PoseidonResult.parse_poseidon_hash_results(rec)[0]
            assert (got.hash_byte, got.hash_id, got.layer_id) == (digest.to_bytes(32, "little"), hid, layer)
    two = R.pack_record(5, 7, 3) + R.pack_record(6, 8, 0)
    assert [(x[1], x[2]) for x in R.parse_poseidon_hash_results(two)] == [(7, 3), (8, 0)]


def test_image_parameter_word_layout():
    """PoseidonImageParametrs::parse_image_params (poseidon_api.rs:256-271): params.to_be_bytes(), packed_struct msb0 bit ranges"""
    def reference_decode(p):
        bits = f"{p:032b}"                            # msb0 string of the big-endian buffer
        f = lambda lo, hi: int(bits[lo:hi + 1], 2)    # noqa: E731
        return f(28, 31), f(20, 27), f(0, 19)

    for cores in (0, 1, 104, 255):
        w = cores << 4                                # what blz_poseidon_loaded_binary_parameters emits
        assert reference_decode(w) == (0, cores, 0)
        m = PoseidonImageParametrs.parse_image_params(w)
        assert (m.hif2_cpu_c_is_stub, m.hif2_cpu_c_number_of_cores, m.hif2_cpu_c_place_holder) == (0, cores, 0)
    src = open(os.path.join(ROOT, "blaze_amd", "csrc", "poseidon.hip")).read()
    assert "out[1] = cores << 4;" in src


def test_matrix_is_applied_row_major_not_transposed():
    """new_i = sum_j M[i][j] s_j with the t^2 MDS words row-major: the tool's Cauchy matrices are symmetric and cannot tell that from
    the transpose, so poseidon_ref is held to the explicit sum on a stream whose matrices are random"""
    r = R.MODULUS["BLS381"]
    words = poseidon_fixtures.with_random_matrices(R.read_instruction_words(SMALL["BLS381"]), r, 3)
    assert check_words("BLS381", TreeMode.TreeC, R.words_bytes(words))["blocks"] == 3
    blocks, _ = R.parse_stream(words)
    for t in (3, 9, 12):
        b = blocks[t]
        m0 = 3 + sum(5 + u * (blocks[u]["rf"] + blocks[u]["rp"]) + u * u for u in (3, 9, 12) if u < t) + 5 + t * (b["rf"] + b["rp"])
        assert all(b["mds"][i][j] == words[m0 + i * t + j] for i in range(t) for j in range(t))         # row-major
        assert any(b["mds"][i][j] != b["mds"][j][i] for i in range(t) for j in range(i))                # not symmetric
        s = list(range(5, 5 + t))
        for rnd in range(b["rf"] + b["rp"]):
            full = not (b["rf"] // 2 <= rnd < b["rf"] // 2 + b["rp"])
            for i in range(t):
                s[i] = (s[i] + b["rc"][rnd][i]) % r
                if full or i == 0:
                    s[i] = s[i] ** 5 % r
            new = [0] * t
            for i in range(t):
                for j in range(t):
                    new[i] = (new[i] + words[m0 + i * t + j] * s[j]) % r
            s = new
        assert R.permute(list(range(5, 5 + t)), b, r) == s
        bt = dict(b, mds=[list(col) for col in zip(*b["mds"])])
        assert R.permute(list(range(5, 5 + t)), bt, r) != s


@pytest.mark.skipif(blaze_amd.lib().blz_device_count() > 0, reason="a GPU is present")
def test_cpp_poseidon_mirror_compiles_and_fails_loudly_without_gpu(tmp_path):
    """include/blaze.hpp's PoseidonClient builds against the C ABI with -Wall -Werror; without a device: FileError (kind 7)"""
    import subprocess
    exe = str(tmp_path / "poseidon_host_example")
    libdir = os.path.join(ROOT, "blaze_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "poseidon_host_example.cpp"), "-L" + libdir, "-lblaze_hip", "-Wl,-rpath," + libdir,
                           "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    p = subprocess.run([exe, FIXTURE, "2"], capture_output=True, text=True)
    assert p.returncode == 1 and "kind 7" in p.stderr


def test_rust_and_cpp_mirrors_bind_every_entry_point():
    hpp = open(os.path.join(ROOT, "include", "blaze.hpp")).read()
    ffi = open(os.path.join(ROOT, "rust", "src", "driver_client", "hip_ffi.rs")).read()
    for f in FUNCTIONS:
        assert "blz_poseidon_" + f in ffi, f
    for need in ("blz_poseidon_new", "blz_poseidon_initialize", "blz_poseidon_set_data", "blz_poseidon_result", "blz_poseidon_raw_results"):
        assert need in hpp, need
    api = open(os.path.join(ROOT, "rust", "src", "ingo_hash", "poseidon_api.rs")).read()
    for fn in ("loaded_binary_parameters", "initialize", "set_data", "start_process", "wait_result", "result", "get_num_of_pending_results",
               "get_raw_results", "get_last_element_sent_to_ring", "get_last_hash_sent_to_host", "log_api_values", "parse_poseidon_hash_results"):
        assert re.search(rf"fn {fn}\s*[<(]", api), fn
    assert os.path.exists(os.path.join(ROOT, "rust", "tests", "integration_poseidon.rs"))
    assert "out of scope" not in open(os.path.join(ROOT, "rust", "Cargo.toml")).read().split("[package]")[0].replace("FPGA shell management is out of scope", "")
