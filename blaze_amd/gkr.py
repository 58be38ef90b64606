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

A FRACTION tree (blz_ntt_gkr_prove_frac, NTTClient.gkr_prove_frac; logUp-GKR) has four tables a layer - P_lo, P_hi, Q_lo, Q_hi - and
two claims, P(tau) and Q(tau).  Layer j >= 1 first draws lambda_j from the transcript (a step that absorbs nothing) and proves
P(tau) + lambda_j Q(tau) = sum_p eq(tau, p) (P_lo Q_hi + P_hi Q_lo + lambda_j Q_lo Q_hi)  by the same sumcheck; layer 0 is held to
root_p = P_lo Q_hi + P_hi Q_lo and root_q = Q_lo Q_hi directly.  rounds and points are laid out as above, and

    claims   4 m words               row j: (P_lo_f, P_hi_f, Q_lo_f, Q_hi_f) at word 4 j
    lambdas  m words                 word j >= 1: lambda_j; word 0 is never written
"""
from collections import namedtuple

from . import fiat_shamir

WORD = fiat_shamir.WORD
TAIL_LEN = 512   # GKR_TAIL_LEN: a layer's rounds at this live length and below run inside one block of the fused path

Layout = namedtuple("Layout", "m rounds_words points_words claims_words weight_words rounds points claims")
LayoutFrac = namedtuple("LayoutFrac", "m rounds_words points_words claims_words lambdas_words weight_words rounds points claims")


def layout(m: int) -> Layout:
    """The word offsets of the op's outputs for a tree over 2^m leaves, m >= 1: rounds[j] is the word of layer j's round 0 (round
    i is 3 i words further; layer 0 has none), points[j] the word of row j (j + 1 words), claims[j] the word of row j (2 words);
    the *_words are the sizes, weight_words the scratch for the weight."""
    m = int(m)
    if m < 1:
        raise ValueError(f"a product tree has 2^m leaves with m >= 1, m = {m} given")
    return Layout(m, 3 * m * (m - 1) // 2, m * (m + 1) // 2, 2 * m, max((1 << m) // 4, 1),
                  tuple(3 * (j * (j - 1) // 2) for j in range(m)), tuple(j * (j + 1) // 2 for j in range(m)), tuple(2 * j for j in range(m)))


def layout_frac(m: int) -> LayoutFrac:
    """The word offsets of blz_ntt_gkr_prove_frac's outputs for trees over 2^m leaves, m >= 1: rounds[j] and points[j] as in
    layout(m), claims[j] = 4 j the word of row j (four words); lambdas_words = m, word j holding lambda_j."""
    m = int(m)
    if m < 1:
        raise ValueError(f"a fraction tree has 2^m leaves with m >= 1, m = {m} given")
    return LayoutFrac(m, 3 * m * (m - 1) // 2, m * (m + 1) // 2, 4 * m, m, max((1 << m) // 4, 1),
                      tuple(3 * (j * (j - 1) // 2) for j in range(m)), tuple(j * (j + 1) // 2 for j in range(m)), tuple(4 * j for j in range(m)))


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


def verify_fraction(field: str, m: int, root_p, root_q, state, rounds, points, claims, lambdas):
    """Verify what NTTClient.gkr_prove_frac wrote for trees over 2^m leaves with the root fraction root_p / root_q (ints), from
    the transcript state the prover started at (32 bytes).  `rounds`, `points`, `claims`, `lambdas` are the four outputs as
    downloaded (bytes) or as lists of ints; word 0 of `lambdas` is not looked at.  Layer 0 is held to root_p = P_lo Q_hi + P_hi
    Q_lo and root_q = Q_lo Q_hi; every lambda, challenge and rho is derived again with fiat_shamir.absorb and compared; every
    round is held to s(0) + s(1) = claim, every layer's end to c (P_lo_f Q_hi_f + P_hi_f Q_lo_f + lambda Q_lo_f Q_hi_f) = claim.
    Raises ValueError naming the layer (and round) at the first mismatch.  Returns (final state, point, (claim_p, claim_q)): the
    sum of fractions is proven if the claims are the multilinear extensions of the numerators and of the denominators at `point`
    (m words, word i paired with bit i of the leaf index), which is the caller's to check."""
    lay = layout_frac(m)
    r = fiat_shamir.MODULUS[field]
    rounds = _words(rounds, lay.rounds_words, "rounds")
    points = _words(points, lay.points_words, "points")
    claims = _words(claims, lay.claims_words, "claims")
    lambdas = [0] + _words(lambdas, lay.lambdas_words, "lambdas")[1:]
    state = bytes(state)
    inv2 = pow(2, -1, r)
    claim_p, claim_q, tau = int(root_p) % r, int(root_q) % r, []
    for j in range(m):
        row = points[lay.points[j]:lay.points[j] + j + 1]
        p_lo, p_hi, q_lo, q_hi = claims[lay.claims[j]:lay.claims[j] + 4]
        if j == 0:
            if (p_lo * q_hi + p_hi * q_lo) % r != claim_p:
                raise ValueError("layer 0: the root numerator is not P_lo Q_hi + P_hi Q_lo of its children")
            if q_lo * q_hi % r != claim_q:
                raise ValueError("layer 0: the root denominator is not the product of its children")
        else:
            state, lam = fiat_shamir.absorb(state, [], field)
            if lam != lambdas[j]:
                raise ValueError(f"layer {j}: lambda is not the transcript's")
            claim = (claim_p + lam * claim_q) % r
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
            if c * (p_lo * q_hi + p_hi * q_lo + lam * q_lo * q_hi) % r != claim:
                raise ValueError(f"layer {j}: eq(tau, z) (P_lo_f Q_hi_f + P_hi_f Q_lo_f + lambda Q_lo_f Q_hi_f) is not the claim")
        state, rho = fiat_shamir.absorb(state, [p_lo, p_hi, q_lo, q_hi], field)
        if rho != row[j]:
            raise ValueError(f"layer {j}: the challenge behind the claims is not the transcript's")
        claim_p = (p_lo + rho * (p_hi - p_lo)) % r
        claim_q = (q_lo + rho * (q_hi - q_lo)) % r
        tau = row
    return state, tau, (claim_p, claim_q)
