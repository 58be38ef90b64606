"""The host mirror of the device transcript (include/blaze_hip.h blz_ntt_fs_challenge), through hashlib: what a verifier runs
to re-derive the challenges of NTTClient.sumcheck_prove from the round polynomials it was sent, and what the tests hold the
device kernel against.

    digest    = SHA3-256(state || w_0 || ... || w_{count-1})      state and words: 32 bytes each, hashed as stored
    new state = digest
    challenge = digest as a little-endian 256-bit integer with every bit from bit bitlen(modulus) - 1 upward cleared

so a challenge is uniform over 2^(bitlen - 1) values and always canonical."""
import hashlib

WORD = 32
MAX_WORDS = 32   # words absorbed behind the state by one step
STATE0 = bytes(WORD)   # the state a fresh transcript may start from; any 32 bytes (a domain separator's digest) serve

# the scalar fields' moduli: the challenge width is one bit below their length
MODULUS = {
    "BLS377": 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001,
    "BLS381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
    "BN254": 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,
}


def challenge_bits(field: str) -> int:
    """Bits a challenge keeps on `field`: 252 on BLS12-377, 254 on BLS12-381, 253 on BN254."""
    return MODULUS[field].bit_length() - 1


def _word(w) -> bytes:
    if isinstance(w, int):
        return w.to_bytes(WORD, "little")
    w = bytes(w)
    if len(w) != WORD:
        raise ValueError(f"a transcript word is {WORD} bytes or a 256-bit unsigned integer, {len(w)} bytes given")
    return w


def absorb(state, words, field: str = "BLS381"):
    """One transcript step: (new state, challenge).  `state` is 32 bytes; `words` is a sequence of at most 32 words - 32 bytes
    each, or ints taken as 256-bit little-endian - or one bytes object holding whole words.  The challenge is an int."""
    state = _word(state)
    if isinstance(words, (bytes, bytearray, memoryview)):
        raw = bytes(words)
        if len(raw) % WORD:
            raise ValueError(f"{len(raw)} bytes are not whole {WORD}-byte words")
        words = [raw[i:i + WORD] for i in range(0, len(raw), WORD)]
    words = [_word(w) for w in words]
    if len(words) > MAX_WORDS:
        raise ValueError(f"one step absorbs at most {MAX_WORDS} words, {len(words)} given")
    digest = hashlib.sha3_256(state + b"".join(words)).digest()
    return digest, int.from_bytes(digest, "little") & ((1 << challenge_bits(field)) - 1)


def challenges(state, rows, field: str = "BLS381"):
    """The prover's transcript over the rows of round polynomials, in order: (final state, [challenge per row])."""
    out = []
    for row in rows:
        state, r = absorb(state, row, field)
        out.append(r)
    return state, out
