"""The host side of the one-call GKR grand product (include/blaze_hip.h blz_ntt_gkr_prove, NTTClient.gkr_prove): where the op
puts its outputs, and the verifier of what it proves, on Python integers and hashlib.

A product tree over 2^m leaves is proven from the root down, layer j = 0 .. m - 1.  Layer j has two tables lo and hi of 2^j words
and a point tau, row j - 1 of the points; the prover shows  claim_j = sum_p eq(tau, p) lo[p] hi[p]  by a sumcheck whose round
polynomials are sent without the eq factor, s_i(X) = c eq(tau_{j-1-i}, X) u_i(X), then sends (lo_f, hi_f), the tables at the
challenges, and the next claim is lo_f + rho (hi_f - lo_f) at the point (challenges in bit order, rho).  After the last layer the
claim is the multilinear extension of the leaves at the last point: that pair is what verify_product returns, for the caller to
check against its own commitment to the leaves.

    rounds   3 m (m - 1) / 2 words   round i < j of layer j: three words u_i(0), u_i(1), u_i(2) at word 3 (j (j - 1) / 2 + i)
    points   m (m + 1) / 2 words     row j: j + 1 words at word j (j + 1) / 2 - the j challenges in bit order, then rho_j
    claims   2 m words               row j: (lo_f, hi_f) at words 2 j and 2 j + 1
"""
from collections import namedtuple

from . import fiat_shamir

WORD = fiat_shamir.WORD
TAIL_LEN = 512   # GKR_TAIL_LEN: a layer's rounds at this live length and below run inside one block of the fused path

Layout = namedtuple("Layout", "m rounds_words points_words claims_words weight_words rounds points claims")


def layout(m: int) -> Layout:
    """The word offsets of the op's outputs for a tree over 2^m leaves, m >= 1: rounds[j] is the word of layer j's round 0 (round
    i is 3 i words further; layer 0 has none), points[j] the word of row j (j + 1 words), claims[j] the word of row j (2 words);
    the *_words are the sizes, weight_words the scratch for the weight."""
    m = int(m)
    if m < 1:
        raise ValueError(f"a product tree has 2^m leaves with m >= 1, m = {m} given")
    return Layout(m, 3 * m * (m - 1) // 2, m * (m + 1) // 2, 2 * m, max((1 << m) // 4, 1),
                  tuple(3 * (j * (j - 1) // 2) for j in range(m)), tuple(j * (j + 1) // 2 for j in range(m)), tuple(2 * j for j in range(m)))


def _words(x, count, name):
    """`count` 256-bit integers out of bytes holding whole words, or out of a sequence of integers"""
    if isinstance(x, (bytes, bytearray, memoryview)):
        raw = bytes(x)
        if len(raw) < count * WORD:
            raise ValueError(f"{name}: {len(raw)} bytes, {count} words of {WORD} bytes expected")
        return [int.from_bytes(raw[i * WORD:(i + 1) * WORD], "little") for i in range(count)]
    out = [int(v) for v in x]
    if len(out) < count or any(v < 0 or v >> 256 for v in out[:count]):
        raise ValueError(f"{name}: {count} unsigned 256-bit words expected")
    return out[:count]


def _eq1(t, x, r):
    return (t * x + (1 - t) * (1 - x)) % r


def verify_product(field: str, m: int, root, state, rounds, points, claims):
    """Verify what NTTClient.gkr_prove wrote for a tree over 2^m leaves with the root `root` (an int), from the transcript state
    the prover started at (32 bytes).  `rounds`, `points`, `claims` are the three outputs as downloaded (bytes) or as lists of
    ints.  Every challenge is derived again with fiat_shamir.absorb and compared with `points`; every round is held to
    s(0) + s(1) = claim, every layer's end to claim = eq(tau, z) lo_f hi_f.  Raises ValueError naming the layer (and round) at
    the first mismatch.  Returns (final state, point, claim): the product is proven if claim is the multilinear extension of the
    leaves at `point` (m words, word i paired with bit i of the leaf index), which is the caller's to check."""
    lay = layout(m)
    r = fiat_shamir.MODULUS[field]
    rounds = _words(rounds, lay.rounds_words, "rounds")
    points = _words(points, lay.points_words, "points")
    claims = _words(claims, lay.claims_words, "claims")
    state = bytes(state)
    inv2 = pow(2, -1, r)
    claim, tau = int(root) % r, []
    for j in range(m):
        row = points[lay.points[j]:lay.points[j] + j + 1]
        lo_f, hi_f = claims[lay.claims[j]], claims[lay.claims[j] + 1]
        c = 1   # eq(tau, .) over the variables bound so far
        for i in range(j):
            u = rounds[lay.rounds[j] + 3 * i:lay.rounds[j] + 3 * i + 3]
            t = tau[j - 1 - i]
            if c * ((1 - t) * u[0] + t * u[1]) % r != claim:
                raise ValueError(f"layer {j}, round {i}: s(0) + s(1) is not the claim")
            state, x = fiat_shamir.absorb(state, u, field)
            if x != row[j - 1 - i]:
                raise ValueError(f"layer {j}, round {i}: the challenge is not the transcript's")
            ux = (u[0] * (x - 1) * (x - 2) * inv2 - u[1] * x * (x - 2) + u[2] * x * (x - 1) * inv2) % r
            c = c * _eq1(t, x, r) % r
            claim = c * ux % r
        if c * lo_f * hi_f % r != claim:
            raise ValueError(f"layer {j}: eq(tau, z) lo_f hi_f is not the claim" if j else "layer 0: the root is not the product of its pair")
        state, rho = fiat_shamir.absorb(state, [lo_f, hi_f], field)
        if rho != row[j]:
            raise ValueError(f"layer {j}: the challenge behind the claims is not the transcript's")
        claim = (lo_f + rho * (hi_f - lo_f)) % r
        tau = row
    return state, tau, claim
