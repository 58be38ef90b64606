"""Textbook Poseidon in Python integers: the independent statement of include/blaze_hip.h "Poseidon" the GPU tests compare
with.  Permutation, fixed-arity hash, the octal tree, the 64-byte record and its parser (a transcription of
PoseidonResult::parse_poseidon_hash_results, poseidon_api.rs:42-71), and a CSV reader that mimics load_instructions
(poseidon_api.rs:205-243).  Independent of tools/poseidon_params.py: it only READS what that tool wrote
(tests/poseidon_fixtures.py)."""
import csv

FIELD_ID = {"BLS377": 0, "BLS381": 1, "BN254": 2}
MODULUS = {
    "BLS377": 8444461749428370424248824938781546531375899335154063827935233455917409239041,
    "BLS381": 52435875175126190479447740508185965837690552500527637822603658699938581184513,
    "BN254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
}
MAGIC = int.from_bytes(b"BLZPOSEIDON01", "little")
TREE_C, TREE_D = 0, 1


def read_instruction_words(path):
    """load_instructions: the first line is a header; every record sends its last column, then its second-to-last."""
    words = []
    with open(path, newline="") as f:
        rd = csv.reader(f)
        next(rd)
        for rec in rd:
            words.append(int(rec[-1], 10))
            words.append(int(rec[-2], 10))
    return words


def words_bytes(words):
    return b"".join(int(w).to_bytes(32, "little") for w in words)


def parse_stream(words):
    """{t: dict(t, rf, rp, tag, rc (list of rounds of t constants), mds (t rows))}, field id"""
    assert words[0] == MAGIC
    field, k = words[1], words[2]
    pos, out = 3, {}
    for _ in range(k):
        t, alpha, rf, rp, tag = words[pos:pos + 5]
        assert alpha == 5
        pos += 5
        rc = [words[pos + r * t: pos + (r + 1) * t] for r in range(rf + rp)]
        pos += t * (rf + rp)
        mds = [words[pos + i * t: pos + (i + 1) * t] for i in range(t)]
        pos += t * t
        out[t] = dict(t=t, rf=rf, rp=rp, tag=tag, rc=rc, mds=mds)
    assert all(w == 0 for w in words[pos:]) and len(words) - pos <= 1
    return out, field


def permute(state, blk, r):
    t, rf, rp = blk["t"], blk["rf"], blk["rp"]
    s = [x % r for x in state]
    assert len(s) == t
    for rnd in range(rf + rp):
        full = rnd < rf // 2 or rnd >= rf // 2 + rp
        s = [(x + c) % r for x, c in zip(s, blk["rc"][rnd])]
        if full:
            s = [pow(x, 5, r) for x in s]
        else:
            s[0] = pow(s[0], 5, r)
        s = [sum(m * x for m, x in zip(row, s)) % r for row in blk["mds"]]
    return s


def hash_fixed(inputs, blk, r):
    """H_t(x_1 .. x_(t-1)): state = [tag, x...], one permutation, digest = state[1]"""
    assert len(inputs) == blk["t"] - 1
    return permute([blk["tag"]] + list(inputs), blk, r)[1]


def tree(elements, height, mode, blocks, r):
    """{(layer, id): digest} for every record of the tree"""
    out = {}
    if mode == TREE_C:
        assert len(elements) == 11 * 8 ** (height - 1)
        cur = [hash_fixed(elements[11 * j: 11 * j + 11], blocks[12], r) for j in range(8 ** (height - 1))]
        for j, d in enumerate(cur):
            out[(0, j)] = d
    else:
        assert len(elements) == 8 ** (height - 1)
        cur = list(elements)
    for layer in range(1, height):
        cur = [hash_fixed(cur[8 * i: 8 * i + 8], blocks[9], r) for i in range(len(cur) // 8)]
        for i, d in enumerate(cur):
            out[(layer, i)] = d
    return out


def pack_record(digest, hash_id, layer_id):
    assert 0 <= hash_id < 1 << 30 and 0 <= layer_id < 1 << 10
    return int(digest).to_bytes(32, "little") + (hash_id | (layer_id << 30)).to_bytes(32, "little")


def parse_poseidon_hash_results(data):
    """[(hash bytes, hash_id, layer_id)], step by step as the reference does it (including the overlapping two-byte read)"""
    data = bytes(data)
    assert len(data) % 64 == 0
    out = []
    for k in range(0, len(data), 64):
        element = data[k:k + 64]
        h, hash_data = element[0:32], element[32:]
        hash_first_4_bytes = hash_data[:4]
        hash_2_bytes = hash_data[3:5]
        hash_last_2_bytes = bytearray(4)
        hash_last_2_bytes[:2] = hash_2_bytes
        hash_id = int.from_bytes(hash_first_4_bytes, "little") & 0x3FFFFFFF
        layer_id = int.from_bytes(hash_last_2_bytes, "little") >> 6
        out.append((h, hash_id, layer_id))
    return out


def num_records(height, mode):
    return sum(8 ** (height - 1 - layer) for layer in range(0 if mode == TREE_C else 1, height))
