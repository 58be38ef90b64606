"""What the tests of blz_ntt_gkr_prove_frac share: the C entry point itself, and a fraction-GKR (logUp-GKR) prover on Python
integers - the two trees, the batching challenge, T = P_hi + lambda Q_hi, the equality table, the rounds u_i(0), u_i(1), u_i(2),
the folds and blaze_amd.fiat_shamir for the challenges - written against the protocol in include/blaze_hip.h and not against
blaze_amd/gkr.py, which it is held against.  Also the logUp instance the tests prove: lookups into a table with multiplicities."""
import ctypes as C
import random

import blaze_amd
from blaze_amd import fiat_shamir
from blaze_amd._lib import BlzVecArg
from ntt_gkr_util import eq_table


def raw_fgkr(cl, flags, tree_p, tree_q, a_p, a_q, length, d_weight, d_state, d_rounds, d_points, d_claims, d_lambdas):
    """blz_ntt_gkr_prove_frac itself: the four operands ints (buffers) / DeviceBuffers / BlzVecArgs / None, the six pointers
    addresses (or None)"""
    vs = [x if isinstance(x, BlzVecArg) or x is None else cl._vec_arg(x) for x in (tree_p, tree_q, a_p, a_q)]
    return blaze_amd.lib().blz_ntt_gkr_prove_frac(cl._h, flags, *[None if v is None else C.byref(v) for v in vs], length, d_weight, d_state, d_rounds,
                                                  d_points, d_claims, d_lambdas)


def frac_trees(a_p, a_q, r):
    """The layers of both trees, leaves first (as stored), the layers above canonical: (P, Q)' = (P_lo Q_hi + P_hi Q_lo, Q_lo Q_hi)"""
    lp, lq = [list(a_p)], [list(a_q)]
    while len(lp[-1]) > 1:
        p, q, half = lp[-1], lq[-1], len(lp[-1]) // 2
        lp.append([(p[i] * q[i + half] + p[i + half] * q[i]) % r for i in range(half)])
        lq.append([q[i] * q[i + half] % r for i in range(half)])
    return lp, lq


def prove_ref(field, a_p, a_q, state):
    """The op on Python integers over the 2^m numerators a_p and denominators a_q (any 256-bit words), from the transcript state
    `state`.  Returns (root_p, root_q, rounds, points, claims, lambdas, final state), the four lists laid out as the op lays
    out its outputs; lambdas[0] is None - the op never writes that word."""
    r = fiat_shamir.MODULUS[field]
    m = len(a_p).bit_length() - 1
    assert len(a_p) == len(a_q) == 1 << m and m >= 1
    lp, lq = frac_trees(a_p, a_q, r)
    rounds, points, claims, lambdas, tau = [], [], [], [None], []
    for j in range(m):
        h = 1 << j
        plo, phi = lp[m - 1 - j][:h], lp[m - 1 - j][h:]
        qlo, qhi = lq[m - 1 - j][:h], lq[m - 1 - j][h:]
        z = []
        if j >= 1:
            state, lam = fiat_shamir.absorb(state, [], field)
            lambdas.append(lam)
            tt = [(phi[p] + lam * qhi[p]) % r for p in range(h)]
            tabs = [plo, tt, qlo, qhi]
            w = eq_table(tau[:j - 1], r)
            for _ in range(j):
                half = len(tabs[0]) // 2
                assert len(w) == half
                u = []
                for t in range(3):
                    x = [[tb[p] + t * (tb[p + half] - tb[p]) for p in range(half)] for tb in tabs]
                    u.append(sum(w[p] * (x[0][p] * x[3][p] + x[2][p] * x[1][p]) for p in range(half)) % r)
                rounds += u
                state, c = fiat_shamir.absorb(state, u, field)
                z.append(c)
                tabs = [[(tb[p] + c * (tb[p + half] - tb[p])) % r for p in range(half)] for tb in tabs]
                if half >= 2:
                    w = [(w[q] + w[q + half // 2]) % r for q in range(half // 2)]
            z = z[::-1]   # the top variable is bound first
            row = [tabs[0][0], (tabs[1][0] - lam * tabs[3][0]) % r, tabs[2][0], tabs[3][0]]
        else:
            row = [plo[0], phi[0], qlo[0], qhi[0]]   # as stored
        claims += row
        state, rho = fiat_shamir.absorb(state, row, field)
        tau = z + [rho]
        points += tau
    return lp[m][0], lq[m][0], rounds, points, claims, lambdas, state


def logup_instance(field, k=5, seed=77, bad=False):
    """2^k lookups into a table of 2^k distinct values, as 2^(k+1) fractions: the lookups' 1 / (beta + f_i) and the table's
    - mult_t / (beta + t_t).  Returns (a_p, a_q): the sum is 0 exactly when every lookup is in the table with the multiplicities
    counted; bad: one lookup replaced by a value that is not in the table."""
    r = fiat_shamir.MODULUS[field]
    rng = random.Random(seed)
    n = 1 << k
    table = rng.sample(range(1, 1 << 20), n)
    idx = [rng.randrange(n) for _ in range(n)]
    mult = [idx.count(t) for t in range(n)]
    looked = [table[i] for i in idx]
    if bad:
        looked[3] = (1 << 21) + 5
    beta = rng.randrange(r)
    a_p = [1] * n + [(r - c) % r for c in mult]
    a_q = [(beta + f) % r for f in looked] + [(beta + t) % r for t in table]
    return a_p, a_q
