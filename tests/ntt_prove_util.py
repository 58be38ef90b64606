"""What the tests of blz_ntt_fs_challenge and blz_ntt_sumcheck_prove share: the two C entry points themselves, and the
host-driven sumcheck the one-call prover is held against - the existing single-step ops with a wait_result between them, every
challenge taken from the host mirror of the transcript (blaze_amd/fiat_shamir.py, hashlib) and uploaded."""
import ctypes as C

import blaze_amd
from blaze_amd import DeviceBuffer, fiat_shamir
from blaze_amd._lib import BlzVecArg


def _arg(cl, x):
    return x if isinstance(x, BlzVecArg) or x is None else cl._vec_arg(x)


def raw_fs(cl, d_state, words, count, d_r):
    """blz_ntt_fs_challenge itself: d_state and d_r addresses (or None), words an int (buffer) / DeviceBuffer / BlzVecArg / None"""
    vw = _arg(cl, words)
    return blaze_amd.lib().blz_ntt_fs_challenge(cl._h, d_state, None if vw is None else C.byref(vw), count, d_r)


def raw_prove(cl, gate, tables, weight, points, length, d_state, d_rounds, d_challenges):
    """blz_ntt_sumcheck_prove itself: gate a BlzSumGate (or None), tables ints / DeviceBuffers / BlzVecArgs (or None), weight a
    DeviceBuffer / BlzVecArg / None, the three outputs addresses (or None)"""
    arr = None if tables is None else (BlzVecArg * max(len(tables), 1))(*[_arg(cl, x) for x in tables])
    vw = _arg(cl, weight)
    return blaze_amd.lib().blz_ntt_sumcheck_prove(cl._h, None if gate is None else C.byref(gate), arr, None if vw is None else C.byref(vw), points,
                                                  length, d_state, d_rounds, d_challenges)


def host_loop(cl, field, tables, terms, common, weight, points, length, state):
    """The m + 2 single ops of a sumcheck over `tables` (folded in place, as the ops do) with the host between them: wait_result,
    download the round, hashlib, upload the challenge.  weight None: sumcheck_gate's steps, else zerocheck_gate's.  Returns
    (rounds bytes, [challenges], final state bytes, summed kernel ms)."""
    m = length.bit_length() - 1
    out = DeviceBuffer(0, 32 * points)
    ms = 0.0

    def step(r, live):
        nonlocal ms
        if weight is None:
            cl.sumcheck_gate(tables, terms, common, r=r, points=points, length=live, out=out)
        else:
            cl.zerocheck_gate(tables, terms, weight, common, r=r, points=points, length=live, out=out)
        cl.wait_result()
        ms += cl.last_kernel_ms()
        return bytes(out.download())

    rows, chal = [], []
    row = step(None, length)
    for i in range(m):
        rows.append(row)
        state, x = fiat_shamir.absorb(state, row, field)
        chal.append(x)
        dr = cl.scalar(x)
        if i < m - 1:
            row = step(dr, length >> i)
        else:
            cl.sumcheck_gate(tables, terms, common, r=dr, points=0, length=2)
            cl.wait_result()
            ms += cl.last_kernel_ms()
        dr.free()
    out.free()
    return b"".join(rows), chal, state, ms
