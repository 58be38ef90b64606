"""What the tests of the multilinear ops and of the two sumcheck steps share (blz_ntt_vec_mle_*, blz_ntt_sumcheck_step,
blz_ntt_sumcheck_gate): filler bytes, the challenge words, the fold on Python integers, the interpolation a sumcheck takes its
next claim with, and the driver of the two steps' order-of-checks tests.  The references of the round polynomials are NOT here:
round_ref, gate_ref and sum_gate_ref stay three independent ones, each beside the entry point it checks."""
import random

import pytest

import blaze_amd
from blaze_amd import DriverClientError
from ntt_vec_util import _words


def fill(nwords, seed):
    """Random bytes behind the words a test knows"""
    return random.Random(seed).randbytes(32 * nwords)


def challenges(r, seed):
    """0, 1, r - 1, r + 1 and a random word >= r"""
    big = next(v for v in _words(seed, 16) if v >= r)
    return [0, 1, r - 1, r + 1, big]


def pairs(a, length, low=False):
    """(lo, hi) of every output position: (p, p + length / 2), or (2p, 2p + 1) with low; a is read periodically, as an op reads
    `count` device words."""
    half, cnt = length // 2, len(a)
    if low:
        return [(a[(2 * p) % cnt], a[(2 * p + 1) % cnt]) for p in range(half)]
    return [(a[p % cnt], a[(p + half) % cnt]) for p in range(half)]


def fold_ref(a, r, rr, length, low=False):
    return [(lo + rr * (hi - lo)) % r for lo, hi in pairs(a, length, low)]


def interpolate(s, x, r):
    """The polynomial through (t, s[t]), t < len(s), at x"""
    acc = 0
    for i, si in enumerate(s):
        num = den = 1
        for j in range(len(s)):
            if j != i:
                num = num * (x - j) % r
                den = den * (i - j) % r
        acc += si * num * pow(den, -1, r)
    return acc % r


def check_order_of_checks(cl, cases, flight, good):
    """cases: (what, (attempt, message, busy), (attempt, message, busy)) - a call wrong in two ways, which reports the EARLIER
    check's message, and the later fault alone with its own message, so that the pair is known to hold two faults.  busy: the
    attempt is made while the op flight() starts is running.  Every attempt returns BLZ_ERR_INVALID_PARAM, leaves nothing in
    flight that was not, and good() - a step checked against Python integers - runs behind it."""
    L = blaze_amd.lib()
    for what, *attempts in cases:
        for attempt, message, busy in attempts:
            if busy:
                flight()
            assert attempt() == 4, what
            assert message in L.blz_last_error_message().decode(), (what, L.blz_last_error_message())
            if busy:
                cl.wait_result()
            with pytest.raises(DriverClientError) as ei:
                cl.wait_result()
            assert ei.value.variant == "InvalidPrimitiveParam", what
            good()
