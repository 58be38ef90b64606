#!/usr/bin/env python3
"""Write a Poseidon instruction CSV for blz_poseidon_initialize (include/blaze_hip.h "THE INSTRUCTION STREAM").

    python tools/poseidon_params.py --field BLS381 --block 9,8,57 --block 12,8,57 -o params.csv

A convenience for callers and the source of the tests' parameter files (tests/poseidon_fixtures.py pins its output by digest).  It is THIS PROJECT'S transcription of the
parameter generation of the Poseidon paper (Grassi, Khovratovich, Rechberger, Roy, Schofnegger), written from its
description: neither the paper's reference script nor its published constants were at hand, equality with them is not
claimed, and the output is not a certified instance.  The library hashes with whatever instance the stream carries.

Word stream (each word a field element, decimal in the CSV):
    magic, field, K, then K blocks of:  t, alpha = 5, R_F, R_P, tag_t, t (R_F + R_P) round constants, t^2 MDS entries (row-major)
    and one zero word if the count is odd.
CSV: a header line, then one record per word pair: `row, word[2 i + 1], word[2 i]` - load_instructions of the reference
(poseidon_api.rs:205-243) sends a record's LAST column first and its SECOND-TO-LAST column second.

Round constants: an 80-bit Grain LFSR, bits b0 .. b79 (b0 is the oldest), initialised MSB-first with
    b0..b1   = 0 1            field type: prime field
    b2..b5   = 0 0 0 0        S-box type: x^alpha
    b6..b17  = field bits n   (12 bits)
    b18..b29 = t              (12 bits)
    b30..b39 = R_F            (10 bits)
    b40..b49 = R_P            (10 bits)
    b50..b79 = 1 ... 1        (30 ones)
update   b(i+80) = b(i+62) ^ b(i+51) ^ b(i+38) ^ b(i+23) ^ b(i+13) ^ b(i); the first 160 output bits are discarded; after that
bits are drawn in pairs - first bit 1: the second bit is output; first bit 0: the pair is dropped.  A field element is n output
bits, most significant first; a value >= r is rejected and the next n bits are drawn (rejection sampling).

MDS matrix: Cauchy, M[i][j] = 1 / (x_i + y_j) mod r with x_i = i, y_j = t + j (0 <= i, j < t).  The tool CLAIMS, and checks
before it writes: M is invertible mod r, and so is M without its row 0 and column 0 (the matrix the optimised partial rounds
would start from).
tag_t = 2^(t - 1) - 1.
"""
import argparse
import sys

MAGIC = int.from_bytes(b"BLZPOSEIDON01", "little")
FIELDS = {   # name: (enum blz_curve, r)
    "BLS377": (0, 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001),
    "BLS381": (1, 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001),
    "BN254": (2, 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001),
}


class Grain:
    def __init__(self, n_bits, t, rf, rp):
        bits = []
        for value, width in ((1, 2), (0, 4), (n_bits, 12), (t, 12), (rf, 10), (rp, 10), ((1 << 30) - 1, 30)):
            bits += [(value >> (width - 1 - k)) & 1 for k in range(width)]
        assert len(bits) == 80
        self.s = bits
        for _ in range(160):
            self._step()

    def _step(self):
        s = self.s
        b = s[62] ^ s[51] ^ s[38] ^ s[23] ^ s[13] ^ s[0]
        self.s = s[1:] + [b]
        return b

    def bit(self):
        while True:
            first, second = self._step(), self._step()
            if first:
                return second

    def element(self, n_bits, r):
        while True:
            v = 0
            for _ in range(n_bits):
                v = (v << 1) | self.bit()
            if v < r:
                return v


def cauchy(t, r):
    return [[pow(i + t + j, -1, r) for j in range(t)] for i in range(t)]


def invertible(m, r):
    """Gaussian elimination mod r"""
    a = [row[:] for row in m]
    n = len(a)
    for c in range(n):
        p = next((k for k in range(c, n) if a[k][c] % r), None)
        if p is None:
            return False
        a[c], a[p] = a[p], a[c]
        inv = pow(a[c][c], -1, r)
        for k in range(c + 1, n):
            f = a[k][c] * inv % r
            if f:
                a[k] = [(x - f * y) % r for x, y in zip(a[k], a[c])]
    return True


def block_words(r, t, rf, rp):
    if not (2 <= t <= 16) or rf < 2 or rf % 2 or rp < 0:
        raise ValueError(f"block (t, R_F, R_P) = ({t}, {rf}, {rp}): 2 <= t <= 16, R_F even and >= 2")
    g = Grain(r.bit_length(), t, rf, rp)
    rc = [g.element(r.bit_length(), r) for _ in range(t * (rf + rp))]
    m = cauchy(t, r)
    if not invertible(m, r) or not invertible([row[1:] for row in m[1:]], r):
        raise ValueError(f"t = {t}: the Cauchy matrix or its lower-right minor is singular")
    return [t, 5, rf, rp, (1 << (t - 1)) - 1] + rc + [x for row in m for x in row]


def generate(field, blocks):
    """The word stream (a list of ints, even length) for `field` ("BLS381" ...) and blocks [(t, R_F, R_P), ...]."""
    fid, r = FIELDS[field]
    words = [MAGIC, fid, len(blocks)]
    for t, rf, rp in blocks:
        words += block_words(r, t, rf, rp)
    if len(words) % 2:
        words.append(0)
    return words


def csv_text(words):
    assert len(words) % 2 == 0
    lines = ["row,second_word,first_word"]
    lines += [f"{i},{words[2 * i + 1]},{words[2 * i]}" for i in range(len(words) // 2)]
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--field", choices=sorted(FIELDS), default="BLS381")
    ap.add_argument("--block", action="append", required=True, metavar="T,RF,RP", help="one block per width, e.g. 9,8,57")
    ap.add_argument("-o", "--output", default="-")
    a = ap.parse_args(argv)
    blocks = [tuple(int(x) for x in b.split(",")) for b in a.block]
    text = csv_text(generate(a.field, blocks))
    if a.output == "-":
        sys.stdout.write(text)
    else:
        with open(a.output, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
