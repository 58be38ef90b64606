"""The on-device transcript (blz_ntt_fs_challenge) and the one-call prover (blz_ntt_sumcheck_prove) on the device.  The
transcript is held against hashlib through the host mirror (blaze_amd/fiat_shamir.py); the prover against the host-driven loop of
the existing single-step ops on copies of the same inputs (tests/ntt_prove_util.py), byte for byte - rounds, challenges, state,
every byte of every table and of the weight - and, end to end, against a Python verifier that knows nothing but the rounds, the
gate and the original tables.  Then the refusals, their order, and the in-flight rules."""
import ctypes as C
import random

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError, fiat_shamir
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_gate_util import CATALOGUE, gate_inputs, gate_value, make_gate
from ntt_mle_util import fill, interpolate
from ntt_prove_util import host_loop, raw_fs, raw_prove
from ntt_spmv_util import _inputs
from ntt_vec_util import FIELDS, TOP, _client, _dev, _pack, _unpack, _words
from ntt_zerocheck_util import PLONK8_TERMS, R1CS3_TERMS, eq1
from oracle import pyref

pytestmark = pytest.mark.gpu
COUNTS = (0, 1, 3, 4, 6, 16, 17, 32)
# (name, ntables, terms, common, weighted, points): R1CS and the eight-table PLONK gate as zerochecks, the catalogue's R1CS with
# its eq as a common factor and no weight, one table at one point
G2 = CATALOGUE["G2"]
GATES = (("R1CS", 3, R1CS3_TERMS, None, True, 3), ("PLONK", 8, PLONK8_TERMS, None, True, 4), ("G2", G2[0], G2[1], G2[2], False, 4),
         ("one table", 1, [(1, [0])], None, False, 1))
# (log n, len): no step with r; one quad; two quads; exactly one block with r, d_out written directly; workspace and finish; a
# live length below n; 4096 on a 2^12 handle (BLS12-381 alone)
SIZES = [(1, 2), (2, 4), (3, 8), (10, 1024), (11, 2048), (11, 512)]
CASES = [(f, logn, length) for logn, length in SIZES for f in FIELDS] + [("BLS381", 12, 4096)]


def _err():
    return blaze_amd.lib().blz_last_error_message().decode()


@pytest.mark.parametrize("field", FIELDS)
def test_fs_challenge_against_the_host_mirror(gpu, field):
    """Every count on either side of the 136-byte rate (3 | 4), with the padding in a block of its own (16) and the most (32), from
    a transform buffer and from device words that hold 0, r - 1, r and 2^256 - 1 among random words - hashed as stored, nothing
    reduced; three calls chained through one state, the second with d_r NULL; the 32 bytes on both sides of the state and of d_r
    keep their value; the challenge is below 2^(bits - 1)."""
    r = pyref.CURVES[field]["r"]
    assert fiat_shamir.MODULUS[field] == r
    bits = r.bit_length()
    logn = 5
    cl = _client(field, logn)
    vals = [0, r - 1, r, TOP] + _words(900 + len(field), 28)
    vals = vals[2:] + vals[:2]
    data = _pack(vals)
    words = _dev(data)
    cl.set_data(NTTInput(1, data[64:] + data[:64]))
    sources = ((words, data), (1, data[64:] + data[:64]))
    guard = DeviceBuffer(0, 32 * 5)   # guard | state | guard | r | guard
    rng = random.Random(len(field))
    for count in COUNTS:
        for src, raw in sources:
            state = rng.randbytes(32)
            gfill = fill(5, count + 3)
            guard.upload(gfill[:32] + state + gfill[64:])
            got_r = []
            for call, with_r in enumerate((True, False, True)):
                assert raw_fs(cl, guard.ptr + 32, src if count else None, count, guard.ptr + 96 if with_r else None) == 0, _err()
                cl.wait_result()
                state, x = fiat_shamir.absorb(state, raw[:32 * count], field)
                g = bytes(guard.download())
                if with_r:
                    got_r = g[96:128]
                    assert got_r == x.to_bytes(32, "little"), (count, call)
                    assert x < 1 << (bits - 1) and x < r
                assert g == gfill[:32] + state + gfill[64:96] + (got_r or gfill[96:128]) + gfill[128:], (count, call)
        assert cl.last_kernel_ms() > 0
    # the Python client: count defaults to all of a DeviceBuffer, r is handed back
    state0 = bytes(range(32))
    d_state, d_r, four = _dev(state0), DeviceBuffer(0, 32), _dev(data[:128])
    assert cl.fs_challenge(d_state, four, r=d_r) is d_r
    cl.wait_result()
    want_state, want_r = fiat_shamir.absorb(state0, data[:128], field)
    assert bytes(d_state.download()) == want_state and bytes(d_r.download()) == want_r.to_bytes(32, "little")
    assert cl.fs_challenge(d_state) is None   # no words, no challenge: the state is hashed alone
    cl.wait_result()
    assert bytes(d_state.download()) == fiat_shamir.absorb(want_state, b"", field)[0]
    assert bytes(words.download()) == data and bytes(cl.result(1)) == data[64:] + data[:64]
    cl.close()
    for d in (words, guard, d_state, d_r, four):
        d.free()


def _place(cl, devs, buffers, data):
    """Table j's bytes go to transform buffer b where buffers[b] == j, else to devs[j]; returns the table operands"""
    tabs = []
    for j, b in enumerate(data):
        if j in buffers:
            cl.set_data(NTTInput(buffers.index(j), b))
            tabs.append(buffers.index(j))
        else:
            devs[j].upload(b)
            tabs.append(devs[j])
    return tabs


def _table_bytes(cl, tabs):
    return [bytes(t.download()) if isinstance(t, DeviceBuffer) else bytes(cl.result(t)) for t in tabs] + [bytes(cl.result(0)), bytes(cl.result(1))]


@pytest.mark.parametrize("field,logn,length", CASES)
def test_prove_equals_the_host_driven_loop(gpu, field, logn, length):
    """Four gates through ONE call and through the m + 2 single ops with the host between them, on copies of the same inputs: two
    tables in the transform buffers (where the gate has two), the others in device words of n words, the weight in len / 2 words
    or in n by turns, random bytes behind the live words.  Equal byte for byte: the rounds, the challenges, the final state,
    every table - both transform buffers whole -, the weight; and the words around the three outputs keep their bytes."""
    n, m = 1 << logn, length.bit_length() - 1
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    devs = [DeviceBuffer(0, 32 * n) for _ in range(8)]
    wdev = [DeviceBuffer(0, 32 * max(length // 2, 1)), DeviceBuffer(0, 32 * n)]
    for turn, (name, nt, terms, common, weighted, points) in enumerate(GATES):
        vals = gate_inputs(r, nt, length, 9100 * logn + 100 * turn + len(field) + length)
        before = [_pack(v) + fill(n - length, turn * 8 + j) for j, v in enumerate(vals)]
        buffers = [turn % nt, (turn + 3) % nt] if nt > 1 else ([0] if turn % 2 == 0 else [])
        wd = wdev[turn % 2] if weighted else None
        wbefore = b""
        if weighted:
            wv = _inputs(r, length // 2, 9150 * logn + turn + len(field))
            wbefore = _pack(wv[turn % len(wv):] + wv[:turn % len(wv)]) + fill(wd.nbytes // 32 - length // 2, turn + 31)
        state0 = random.Random(turn + logn).randbytes(32)
        # guard | state | guard | rounds | guard | challenges | guard
        at_rounds, at_chal = 3, 4 + m * points
        total = at_chal + m + 1
        gfill = fill(total, turn + 5)
        gbytes = gfill[:32] + state0 + gfill[64:]
        guard = _dev(gbytes)
        tabs = _place(cl, devs, buffers, before)
        if weighted:
            wd.upload(wbefore)
        gate = make_gate(nt, terms, common)
        assert raw_prove(cl, gate, tabs, wd, points, length, guard.ptr + 32, guard.ptr + 32 * at_rounds, guard.ptr + 32 * at_chal) == 0, (name, _err())
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        g = bytes(guard.download())
        one_tables = _table_bytes(cl, tabs)
        one_weight = bytes(wd.download()) if weighted else b""
        # the host-driven loop on copies of the same inputs
        tabs = _place(cl, devs, buffers, before)
        if weighted:
            wd.upload(wbefore)
        rows, chal, state, _ = host_loop(cl, field, tabs, terms, common, wd, points, length, state0)
        assert len(rows) == 32 * m * points and len(chal) == m
        want = gfill[:32] + state + gfill[64:96] + rows + gfill[32 * (at_rounds + m * points):32 * at_chal] + _pack(chal) + gfill[32 * (at_chal + m):]
        assert g[32:64] == state, (name, "final state")
        assert g[32 * at_rounds:32 * (at_rounds + m * points)] == rows, (name, "rounds")
        assert g[32 * at_chal:32 * (at_chal + m)] == _pack(chal), (name, "challenges")
        assert g == want, (name, "the words around the three outputs")
        assert one_tables == _table_bytes(cl, tabs), (name, "tables")
        assert one_weight == (bytes(wd.download()) if weighted else b""), (name, "weight")
        # and no more was written than the single ops write: bytes behind len / 2 words of a table, len / 4 of the weight
        for j, t in enumerate(one_tables[:nt]):
            assert t[16 * length:] == before[j][16 * length:], (name, j)
        if weighted:
            assert one_weight[8 * length:] == wbefore[8 * length:], name
        guard.free()
    cl.close()
    for d in devs + wdev:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_plonk_zerocheck_proved_in_one_call(gpu, field):
    """The satisfied 2^10-row PLONK circuit of tests/test_gpu_ntt_zerocheck.py: eight tables, the weight eq(tau_0 .. tau_8, .), 4
    points a round, ONE call.  The verifier is Python: it re-derives every challenge from the downloaded rounds with hashlib,
    rebuilds s_i(t) = c_i eq(tau_{m-1-i}, t) u_i(t), checks s_i(0) + s_i(1) against the running claim - 0 at first - and the last
    claim against the eight bound words, which are the original tables at the challenges.  One flipped witness word: round 0's sum
    is not 0."""
    m = 10
    n = 1 << m
    r = pyref.CURVES[field]["r"]
    rng = random.Random(len(field) + 390)
    qL, qR, qM, qC, a, b = ([rng.randrange(r) for _ in range(n)] for _ in range(6))
    qO = [rng.randrange(1, r) for _ in range(n)]
    c = [(qL[p] * a[p] + qR[p] * b[p] + qM[p] * a[p] * b[p] + qC[p]) * pow(qO[p], -1, r) % r for p in range(n)]
    tau = _words(len(field) + 391, m)
    cl = _client(field, m)
    point, d_w = _dev(_pack(tau)), DeviceBuffer(0, 32 * (n // 2))
    cl.vec_mle_eq(d_w, point, m - 1); cl.wait_result()
    orig = [qL, qR, qM, qO, qC, a, b, c]
    devs = [_dev(_pack(v)) for v in (qL, qR, qM, qO, qC, c)]
    cl.set_data(NTTInput(0, _pack(a)))
    cl.set_data(NTTInput(1, _pack(b)))
    tabs = devs[:5] + [0, 1, devs[5]]
    state0 = bytes(32)
    d_state = _dev(state0)
    rounds, d_chal = cl.sumcheck_prove(tabs, PLONK8_TERMS, d_state, weight=d_w)
    assert rounds.nbytes == 32 * 4 * m and d_chal.nbytes == 32 * m
    cl.wait_result()
    sent = bytes(rounds.download())
    rows = [sent[128 * i:128 * (i + 1)] for i in range(m)]
    state, chal = fiat_shamir.challenges(state0, rows, field)
    assert _unpack(d_chal.download()) == chal and bytes(d_state.download()) == state
    claim, coef = 0, 1
    for i, x in enumerate(chal):
        u = _unpack(rows[i])
        top = tau[m - 1 - i]
        s = [coef * eq1(top, t, r) * (u[t] if t < 4 else interpolate(u, t, r)) % r for t in range(5)]
        assert (s[0] + s[1]) % r == claim, (i, "s(0) + s(1) = claim")
        claim = interpolate(s, x, r)
        coef = coef * eq1(top, x, r) % r
    finals = [_unpack((bytes(t.download(32)) if isinstance(t, DeviceBuffer) else bytes(cl.result(t))[:32]))[0] for t in tabs]
    assert claim == coef * gate_value(finals, PLONK8_TERMS, None, r) % r

    def at_challenges(table):
        for x in chal:
            h = len(table) // 2
            table = [(table[p] + x * (table[p + h] - table[p])) % r for p in range(h)]
        return table[0]

    assert finals == [at_challenges(t) for t in orig]
    # one witness word flipped: the circuit is not satisfied and round 0 says so
    bad = list(c)
    bad[rng.randrange(n)] ^= 1
    for t, v in zip(devs, (qL, qR, qM, qO, qC, bad)):
        t.upload(_pack(v))
    cl.set_data(NTTInput(0, _pack(a)))
    cl.set_data(NTTInput(1, _pack(b)))
    cl.vec_mle_eq(d_w, point, m - 1); cl.wait_result()
    d_state.upload(state0)
    cl.sumcheck_prove(tabs, PLONK8_TERMS, d_state, weight=d_w, rounds=rounds, challenges=d_chal)
    cl.wait_result()
    u = _unpack(rounds.download(128))
    s = [eq1(tau[m - 1], t, r) * u[t] % r for t in range(2)]
    assert (s[0] + s[1]) % r != 0
    cl.close()
    for d in devs + [point, d_w, d_state, rounds, d_chal]:
        d.free()


def test_refusals_and_the_order_of_checks(gpu):
    """Every refusal returns BLZ_ERR_INVALID_PARAM with its own message, leaves nothing in flight and changes no byte; a call wrong
    in two ways reports the earlier check."""
    field, logn = "BLS381", 4
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    L = blaze_amd.lib()
    ab, bb = _pack(_inputs(r, n, 1)), _pack(_inputs(r, n, 2))
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb))
    cb, wb = _pack(_inputs(r, 2 * n, 3)), _pack(_inputs(r, n, 4))
    words, weight = _dev(cb), _dev(wb)
    outs_b = fill(64, 5)
    outs = _dev(outs_b)   # state at word 0, rounds at 8, challenges at 40
    st, ro, ch = outs.ptr, outs.ptr + 32 * 8, outs.ptr + 32 * 40
    host = (C.c_char * 64)()   # host memory where a device word belongs
    host_ptr = C.addressof(host)
    gate3 = make_gate(3, R1CS3_TERMS, None)
    w3 = words.view(0, 32 * n)          # the third table: words [0, n) of `words`
    w3b = words.view(32 * n, 32 * n)    # words [n, 2n)
    crossing = BlzVecArg(words.ptr + 32 * (n // 2), 0, 0, n)   # words [n / 2, 3n / 2): meets both
    half_w = weight.view(0, 32 * (n // 4))
    period = words.view(0, 32 * (n // 2))
    tabs3 = [0, 1, w3]

    def prove(gate=gate3, tables=tabs3, w=weight, points=3, length=n, s=st, rd=ro, c=ch):
        return lambda: raw_prove(cl, gate, tables, w, points, length, s, rd, c)

    def fs(s=st, w=w3, count=3, rr=ro):
        return lambda: raw_fs(cl, s, w, count, rr)

    junk = make_gate(3, R1CS3_TERMS, 7)
    refused = [
        (lambda: L.blz_ntt_sumcheck_prove(None, None, None, None, 0, 0, None, None, None), "null handle"),
        (lambda: L.blz_ntt_fs_challenge(None, None, None, 99, None), "null handle"),
        (prove(gate=None), "gate is NULL"), (prove(tables=None), "tables is NULL"), (prove(s=None), "d_state is NULL"),
        (prove(rd=None), "d_rounds is NULL"), (prove(c=None), "d_challenges is NULL"),
        (prove(gate=junk), "gate: common 7"),
        (prove(points=0), "points 0 is not in [1, 6]"), (prove(points=7), "points 7 is not in [1, 6]"),
        (prove(length=1), "len 1:"), (prove(length=12), "len 12:"), (prove(length=2 * n), f"len {2 * n}:"),
        (prove(tables=[0, 1, period]), "operand tables[2]: 8 words, read periodically over len 16"),
        (prove(tables=[0, w3, crossing]), "tables[1] and tables[2] meet in their first len words"),
        (prove(tables=[0, 0, w3]), "tables[0] and tables[1] meet in their first len words"),
        (prove(w=half_w), "operand weight: 4 words, a step with r sums len / 2 = 8"),
        (prove(w=BlzVecArg(None, 1, 0, 0)), "the weight is device words"),
        (prove(w=w3b, tables=[0, 1, crossing]), "the weight's first len / 2 words meet the first len words of tables[2]"),
        (prove(s=words.ptr + 32), "d_state lies in the live words of tables[2]"),
        (prove(rd=weight.ptr + 64), "d_rounds overlaps the words of the weight"),
        (prove(c=ro + 32 * 11), "d_challenges overlaps d_rounds"), (prove(rd=st), "d_rounds overlaps d_state"),
        (prove(s=st + 8), "d_state: the pointer is not 16-byte aligned"), (prove(s=host_ptr), "d_state: the pointer is not"),
        (prove(c=outs.ptr + 32 * 62), "d_challenges: 4 elements run past the end"),
        (fs(count=33), "count 33 is not in [0, 32]"), (fs(s=None), "null d_state"), (fs(w=None), "words is NULL"),
        (fs(s=st + 8), "d_state is not 16-byte aligned"), (fs(s=host_ptr), "d_state is not"), (fs(rr=st), "d_r overlaps d_state"),
        (fs(w=half_w, count=5), "operand words: 4 words"), (fs(s=words.ptr + 64), "d_state lies in the words absorbed"),
        (fs(rr=words.ptr), "d_r lies in the words absorbed"), (fs(w=BlzVecArg(None, 2, 0, 0)), "buf must be 0 or 1"),
    ]
    # wrong in two ways: the earlier check speaks
    refused += [
        (prove(gate=None, points=9), "gate is NULL"), (prove(gate=junk, points=9), "gate: common 7"), (prove(points=9, length=12), "points 9"),
        (prove(length=12, w=BlzVecArg(None, 1, 0, 0)), "the weight is device words"), (prove(length=12, s=st + 8), "len 12:"),
        (prove(tables=[0, 1, period], s=st + 8), "read periodically"), (prove(w=half_w, rd=st), "operand weight: 4 words"),
        (prove(s=st + 8, rd=st), "d_state: the pointer is not 16-byte aligned"), (fs(count=33, s=None), "null d_state"),
        (fs(count=33, w=None), "count 33"), (fs(w=half_w, count=5, s=st + 8), "operand words: 4 words"),
    ]

    def unchanged():
        with pytest.raises(DriverClientError) as ei:
            cl.wait_result()   # nothing is in flight
        assert ei.value.variant == "InvalidPrimitiveParam"
        assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
        assert bytes(words.download()) == cb and bytes(weight.download()) == wb and bytes(outs.download()) == outs_b

    for attempt, message in refused:
        assert attempt() == 4, message
        assert message in _err(), (message, _err())
        unchanged()
    # an op already in flight: refused behind the argument checks, ahead of the operands'
    for attempt, message in ((prove(), "already running"), (fs(), "already running"), (prove(points=9), "points 9"), (fs(count=33), "count 33"),
                             (prove(tables=[0, 1, period]), "already running")):
        cl.vec_mle_round(w3)
        assert attempt() == 4 and message in _err(), (message, _err())
        cl.wait_result()
        unchanged()
    # and the good call behind them all
    assert prove()() == 0, _err()
    cl.wait_result()
    got = bytes(outs.download())
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb)); words.upload(cb); weight.upload(wb)
    rows, chal, state, _ = host_loop(cl, field, tabs3, R1CS3_TERMS, None, weight, 3, n, outs_b[:32])
    assert got == state + outs_b[32:256] + rows + outs_b[32 * 20:32 * 40] + _pack(chal) + outs_b[32 * 44:]
    cl.close()
    for d in (words, weight, outs):
        d.free()


def test_in_flight_rules(gpu):
    """While the chain runs over BOTH transform buffers neither can be read, written or exchanged and no op starts; a transcript
    step that reads buffer 0 leaves both readable and buffer 0 unwritable; reset drops the chain, and the handle works afterwards."""
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b, c, w = (_inputs(r, n, 270 + i) for i in range(4))
    ab, bb, cb, wb = _pack(a), _pack(b), _pack(c), _pack(w[:n // 2])
    cl = _client(field, logn)
    words, weight, one_word = _dev(cb), _dev(wb), _dev((7).to_bytes(32, "little"))
    state0 = bytes(range(1, 33))
    d_state = _dev(state0)
    host_out = bytearray(32 * n)
    busy = (lambda: cl.start_process(0), lambda: cl.set_coset(7), lambda: cl.vec_op(NTTClient.MUL, 1, 1, words), lambda: cl.vec_reduce(NTTClient.FOLD_SUM, 0),
            lambda: cl.vec_mle_round(words), lambda: cl.sumcheck_gate([words], [(1, [0])]), lambda: cl.zerocheck_gate([words], [(1, [0])], weight),
            lambda: cl.fs_challenge(d_state, one_word), lambda: cl.sumcheck_prove([words], [(1, [0])], d_state))

    def load():
        cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb)); words.upload(cb); weight.upload(wb); d_state.upload(state0)

    for tabs in ([1, 0, words], [0, 1, words]):
        load()
        rounds, chal = cl.sumcheck_prove(tabs, R1CS3_TERMS, d_state, weight=weight)
        for attempt in busy + (lambda: cl.result(0), lambda: cl.result(1), lambda: cl.set_data(NTTInput(0, ab)), lambda: cl.set_data(NTTInput(1, ab)),
                               lambda: cl.exchange(0, ab, host_out), lambda: cl.exchange(1, ab, host_out)):
            with pytest.raises(DriverClientError) as ei:
                attempt()
            assert ei.value.variant == "InvalidPrimitiveParam"
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        got = (bytes(rounds.download()), _unpack(chal.download()), bytes(d_state.download()), bytes(cl.result(0)), bytes(cl.result(1)))
        load()
        rows, xs, state, _ = host_loop(cl, field, tabs, R1CS3_TERMS, None, weight, 3, n, state0)
        assert got == (rows, xs, state, bytes(cl.result(0)), bytes(cl.result(1)))
        rounds.free(); chal.free()
    # a transcript step over buffer 0: read-only, as for a reduce
    load()
    d_r = cl.fs_challenge(d_state, 0, count=6, r=DeviceBuffer(0, 32))
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == bb
    cl.set_data(NTTInput(1, bb))   # not named
    with pytest.raises(DriverClientError) as ei:
        cl.set_data(NTTInput(0, ab))
    assert ei.value.variant == "InvalidPrimitiveParam" and "buffer 0" in str(ei.value)
    for attempt in busy:
        with pytest.raises(DriverClientError):
            attempt()
    cl.wait_result()
    want_state, want_r = fiat_shamir.absorb(state0, ab[:192], field)
    assert bytes(d_state.download()) == want_state and bytes(d_r.download()) == want_r.to_bytes(32, "little")
    # reset with the chain in flight: nothing is in flight afterwards, and the handle works
    load()
    rounds, chal = cl.sumcheck_prove([0, 1, words], R1CS3_TERMS, d_state, weight=weight)
    cl.reset()
    with pytest.raises(DriverClientError):
        cl.wait_result()
    cl.result(0); cl.result(1)
    load()
    cl.sumcheck_prove([0, 1, words], R1CS3_TERMS, d_state, weight=weight, rounds=rounds, challenges=chal)
    cl.wait_result()
    got = (bytes(rounds.download()), _unpack(chal.download()), bytes(d_state.download()))
    load()
    assert got == host_loop(cl, field, [0, 1, words], R1CS3_TERMS, None, weight, 3, n, state0)[:3]
    cl.close()
    for d in (words, weight, one_word, d_state, d_r, rounds, chal):
        d.free()
