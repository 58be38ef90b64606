"""What the tests of blz_ntt_gkr_prove share: the C entry point itself, and a GKR grand-product prover on Python integers - the
product tree, the equality table, the rounds u_i(0), u_i(1), u_i(2), the folds and blaze_amd.fiat_shamir for the challenges -
written against the protocol in include/blaze_hip.h and not against blaze_amd/gkr.py, which it is held against."""
import ctypes as C

import blaze_amd
from blaze_amd import fiat_shamir
from blaze_amd._lib import BlzVecArg


def raw_gkr(cl, op, flags, tree, a, length, d_weight, d_state, d_rounds, d_points, d_claims):
    """blz_ntt_gkr_prove itself: tree and a ints (buffers) / DeviceBuffers / BlzVecArgs / None, the five pointers addresses (or None)"""
    vt, va = (x if isinstance(x, BlzVecArg) or x is None else cl._vec_arg(x) for x in (tree, a))
    return blaze_amd.lib().blz_ntt_gkr_prove(cl._h, op, flags, None if vt is None else C.byref(vt), None if va is None else C.byref(va), length,
                                             d_weight, d_state, d_rounds, d_points, d_claims)


def eq_table(tau, r):
    """eq(tau, p) for p < 2^len(tau), tau_i paired with bit i"""
    tab = [1]
    for t in tau:
        tab = [v * (1 - t) % r for v in tab] + [v * t % r for v in tab]
    return tab


def mle_at(values, point, r):
    """The multilinear extension of `values` (2^len(point) of them, point_i paired with bit i of the index) at `point`"""
    cur = [v % r for v in values]
    for x in reversed(point):   # the top variable first: (p, p + half)
        half = len(cur) // 2
        cur = [(cur[p] + x * (cur[p + half] - cur[p])) % r for p in range(half)]
    return cur[0]


def prove_ref(field, leaves, state):
    """The op on Python integers over the 2^m words `leaves` (any 256-bit words), from the transcript state `state`.  Returns
    (root, rounds, points, claims, final state), the three lists laid out as the op lays out its outputs."""
    r = fiat_shamir.MODULUS[field]
    m = len(leaves).bit_length() - 1
    assert len(leaves) == 1 << m and m >= 1
    layers = [list(leaves)]   # layer 0 as stored; the layers above canonical
    while len(layers[-1]) > 1:
        cur, half = layers[-1], len(layers[-1]) // 2
        layers.append([cur[p] * cur[p + half] % r for p in range(half)])
    rounds, points, claims, tau = [], [], [], []
    for j in range(m):
        below = layers[m - 1 - j]
        lo, hi = below[:1 << j], below[1 << j:]
        z = []
        if j >= 1:
            w = eq_table(tau[:j - 1], r)
            for _ in range(j):
                half = len(lo) // 2
                assert len(w) == half
                u = [sum(w[p] * (lo[p] + t * (lo[p + half] - lo[p])) * (hi[p] + t * (hi[p + half] - hi[p])) for p in range(half)) % r for t in range(3)]
                rounds += u
                state, x = fiat_shamir.absorb(state, u, field)
                z.append(x)
                lo = [(lo[p] + x * (lo[p + half] - lo[p])) % r for p in range(half)]
                hi = [(hi[p] + x * (hi[p + half] - hi[p])) % r for p in range(half)]
                if half >= 2:
                    w = [(w[q] + w[q + half // 2]) % r for q in range(half // 2)]
            z = z[::-1]   # the top variable is bound first
        claims += [lo[0], hi[0]]
        state, rho = fiat_shamir.absorb(state, [lo[0], hi[0]], field)
        tau = z + [rho]
        points += tau
    return layers[m][0], rounds, points, claims, state
