"""The one-call GKR grand-product prover (blz_ntt_gkr_prove) on the device.  The tree is built by mle_tree in the test.  The fused
path - k_gkr_tail, one block that keeps a layer in LDS - against the chain of existing launches (BLZ_GKR_UNFUSED), byte for byte
on d_rounds, d_points, d_claims and d_state; the chain against the host-driven loop of the single ops; the verifier of
blaze_amd/gkr.py on the fused output; edge words; the bytes that may and may not change; every refusal in the documented order;
the in-flight rules.  Every run carries guard words on both sides of the four outputs and of the weight and checks that the upper
half of every half-layer of the tree and of the leaves, the root and the tree's last word keep their bytes."""
import ctypes as C

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError, fiat_shamir, gkr
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_gkr_util import mle_at, prove_ref, raw_gkr
from ntt_mle_util import fill
from ntt_prove_util import host_loop
from ntt_vec_util import FIELDS, TOP, _client, _dev, _pack, _unpack, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
PROD, FRAC, UNFUSED = NTTClient.TREE_PROD, NTTClient.TREE_FRAC, NTTClient.GKR_UNFUSED
STATE0 = bytes(range(101, 133))
G = 32   # one guard word


def _err():
    return blaze_amd.lib().blz_last_error_message().decode()


def _leaves(field, m, edges=False):
    """Random 256-bit words, more than half of them above the modulus; edges: 0, 1, r - 1, r, r + 1 and 2^256 - 1 twice each among them"""
    r = pyref.CURVES[field]["r"]
    a = _words(52000 + 10 * m + len(field), 1 << m)
    if edges:
        for i, e in enumerate([0, 1, r - 1, r, r + 1, TOP] * 2):
            a[(5 * i + 1) % len(a)] = e   # 5 is odd: twelve distinct places among sixteen
    return a


def _halves(n, j):
    """(buffer is the leaves, word of lo, word of hi, words of each) of layer j's tables"""
    m = n.bit_length() - 1
    k = m - 1 - j
    off = 0 if k == 0 else NTTClient.tree_layer(n, k)[0]
    return k == 0, off, off + (1 << j), 1 << j


def _kept(n, tree0, a0, tree1, a1):
    """Every byte of the tree and of the leaves outside the first half of each half-layer is as it was"""
    m = n.bit_length() - 1
    for j in range(m):
        leaf, lo, hi, h = _halves(n, j)
        before, after = (a0, a1) if leaf else (tree0, tree1)
        for s in (lo, hi):
            assert after[32 * (s + h // 2):32 * (s + h)] == before[32 * (s + h // 2):32 * (s + h)], ("upper half", j, s)
    assert tree1[32 * (n - 2):] == tree0[32 * (n - 2):], "the root and the word behind it"
    assert len(a1) == len(a0) and len(tree1) == len(tree0)


class _Outs:
    """The four outputs and the weight, each between two guard words of random bytes, in two allocations"""

    def __init__(self, m, seed, state0=STATE0):
        self.lay = lay = gkr.layout(m)
        sizes = (1, lay.rounds_words, lay.points_words, lay.claims_words)
        self.at, pos = [], 1
        for s in sizes:
            self.at.append(pos)
            pos += s + 1
        self.sizes = sizes
        self.fill, self.wfill = fill(pos, seed), fill(lay.weight_words + 2, seed + 1)
        self.fill = self.fill[:G] + state0 + self.fill[2 * G:]   # the transcript starts from state0
        self.buf, self.wbuf = _dev(self.fill), _dev(self.wfill)
        self.state, self.rounds, self.points, self.claims = (self.buf.view(32 * a, 32 * s) for a, s in zip(self.at, sizes))
        self.weight = self.wbuf.view(G, 32 * lay.weight_words)

    def collect(self):
        """(state, rounds, points, claims) bytes; the guard words are checked on the way"""
        got, wgot = bytes(self.buf.download()), bytes(self.wbuf.download())
        want = bytearray(self.fill)
        out = []
        for a, s in zip(self.at, self.sizes):
            out.append(got[32 * a:32 * (a + s)])
            want[32 * a:32 * (a + s)] = out[-1]
        assert got == bytes(want), "a byte outside the four outputs changed"
        assert wgot[:G] == self.wfill[:G] and wgot[-G:] == self.wfill[-G:], "a guard word of the weight changed"
        return tuple(out)

    def free(self):
        self.buf.free()
        self.wbuf.free()


_RUNS = {}


def _run(field, m, fused, edges=False):
    """One proof over device words, computed once: (state, rounds, points, claims, root)"""
    key = (field, m, fused, edges)
    if key not in _RUNS:
        n = 1 << m
        ab = _pack(_leaves(field, m, edges))
        cl = _client(field, m)
        a, tree, outs = _dev(ab), _dev(fill(n, 60 + m)), _Outs(m, 600 + m)
        cl.mle_tree(tree, a)
        cl.wait_result()
        tree0 = bytes(tree.download())
        cl.gkr_prove(tree, a, outs.state, weight=outs.weight, rounds=outs.rounds, points=outs.points, claims=outs.claims, fused=fused)
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        _kept(n, tree0, ab, bytes(tree.download()), bytes(a.download()))
        _RUNS[key] = outs.collect() + (int.from_bytes(tree0[32 * (n - 2):32 * (n - 1)], "little"),)
        cl.close()
        for d in (a, tree):
            d.free()
        outs.free()
    return _RUNS[key]


# all-fused up to m = 10, one chain step at the layer of 1024, two and three at m = 12 and 13
SIZES = [("BLS381", m) for m in (1, 2, 3, 9, 10, 11, 12, 13)] + [(f, m) for f in ("BLS377", "BN254") for m in (3, 11)]


@pytest.mark.parametrize("field,m", SIZES)
def test_fused_equals_unfused_byte_for_byte(gpu, field, m):
    one, chain = _run(field, m, True), _run(field, m, False)
    for what, x, y in zip(("d_state", "d_rounds", "d_points", "d_claims"), one, chain):
        assert x == y, what
    assert one[0] != STATE0 and one[4] == chain[4]
    r = pyref.CURVES[field]["r"]
    assert all(v < r for part in one[1:4] for v in _unpack(part)) or m == 1   # canonical; at m = 1 the claims are the leaves as stored


def _host_driven(cl, field, n, tree, a, state):
    """The proof by the single ops with the host between them: per layer vec_mle_eq, ntt_prove_util.host_loop over views of the
    layer, a download of the two final words, hashlib.  Returns (state, rounds, points, claims) bytes."""
    m = n.bit_length() - 1
    eq = DeviceBuffer(0, 32 * max(n // 4, 1))
    rounds, points, claims, tau = b"", [], b"", []
    for j in range(m):
        leaf, lo, hi, h = _halves(n, j)
        below = a if leaf else tree
        tl, th = below.view(32 * lo, 32 * h), below.view(32 * hi, 32 * h)
        z = []
        if j >= 1:
            point = _dev(_pack(tau))
            cl.vec_mle_eq(eq, point, j - 1)
            cl.wait_result()
            point.free()
            rows, chal, state, _ = host_loop(cl, field, [tl, th], [(1, [0, 1])], None, eq.view(0, 32 * (h // 2)), 3, h, state)
            rounds += rows
            z = chal[::-1]
        pair = bytes(tl.download(32)) + bytes(th.download(32))
        claims += pair
        state, rho = fiat_shamir.absorb(state, pair, field)
        tau = z + [rho]
        points += tau
    eq.free()
    return state, rounds, _pack(points), claims


@pytest.mark.parametrize("m", (1, 2, 6, 11))
def test_unfused_equals_the_host_driven_loop(gpu, m):
    field, n = "BLS381", 1 << m
    ab = _pack(_leaves(field, m))
    cl = _client(field, m)
    a, tree = _dev(ab), DeviceBuffer(0, 32 * n)
    cl.mle_tree(tree, a)
    cl.wait_result()
    want = _host_driven(cl, field, n, tree, a, STATE0)
    assert _run(field, m, False)[:4] == want
    cl.close()
    for d in (a, tree):
        d.free()


@pytest.mark.parametrize("m", (4, 10, 12))
def test_verifier_accepts_the_fused_output(gpu, m):
    field = "BLS381"
    r = pyref.CURVES[field]["r"]
    leaves = _leaves(field, m)
    state, rounds, points, claims, root = _run(field, m, True)
    prod = 1
    for v in leaves:
        prod = prod * v % r
    assert root == prod
    final, point, claim = gkr.verify_product(field, m, root, STATE0, rounds, points, claims)
    assert final == state and len(point) == m
    assert claim == mle_at(leaves, point, r)
    with pytest.raises(ValueError, match="layer 0"):
        gkr.verify_product(field, m, (root + 1) % r, STATE0, rounds, points, claims)


@pytest.mark.parametrize("field", FIELDS)
def test_prover_on_python_integers_and_edge_words(gpu, field):
    """m = 4: both paths equal the prover written on Python integers, over random words and over leaves that hold 0, 1, r - 1, r,
    r + 1 and 2^256 - 1 twice each - which the fused kernel reads as stored."""
    for edges in (False, True):
        leaves = _leaves(field, 4, edges)
        if edges:
            r = pyref.CURVES[field]["r"]
            assert all(leaves.count(e) >= 2 for e in (0, 1, r - 1, r, r + 1, TOP))
        root, rounds, points, claims, state = prove_ref(field, leaves, STATE0)
        want = (state, _pack(rounds), _pack(points), _pack(claims), root)
        assert _run(field, 4, True, edges) == want, ("fused", edges)
        assert _run(field, 4, False, edges) == want, ("unfused", edges)
    # m = 1: the claims are the two leaves as stored, above the modulus or not
    leaves = [TOP, pyref.CURVES[field]["r"] + 1]
    cl = _client(field, 1)
    for fused in (True, False):
        a, tree, outs = _dev(_pack(leaves)), DeviceBuffer(0, 64), _Outs(1, 77)
        cl.mle_tree(tree, a)
        cl.wait_result()
        cl.gkr_prove(tree, a, outs.state, weight=outs.weight, rounds=outs.rounds, points=outs.points, claims=outs.claims, fused=fused)
        cl.wait_result()
        state, rounds, points, claims = outs.collect()
        root, _, wp, wc, ws = prove_ref(field, leaves, STATE0)
        assert (state, rounds, points, claims) == (ws, b"", _pack(wp), _pack(leaves)) and wc == leaves, fused
        for d in (a, tree):
            d.free()
        outs.free()
    cl.close()


@pytest.mark.parametrize("m", (5, 11))
def test_bytes_buffers_and_views(gpu, m):
    """Guard words and the kept halves are checked by every run (m = 5 and 11, both paths, here).  The same proof with tree and a
    as the handle's two transform buffers, and as two views of one allocation."""
    field, n = "BLS381", 1 << m
    ab = _pack(_leaves(field, m))
    want = {fused: _run(field, m, fused) for fused in (True, False)}
    assert want[True] == want[False]
    cl = _client(field, m)
    both = DeviceBuffer(0, 64 * n)
    for fused in (True, False):
        # the handle's two buffers: the tree in buffer 0, the leaves in buffer 1
        outs = _Outs(m, 900 + m)
        cl.set_data(NTTInput(1, ab))
        cl.set_data(NTTInput(0, fill(n, 5)))
        cl.mle_tree(0, 1)
        cl.wait_result()
        tree0 = bytes(cl.result(0))
        cl.gkr_prove(0, 1, outs.state, weight=outs.weight, rounds=outs.rounds, points=outs.points, claims=outs.claims, fused=fused)
        cl.wait_result()
        _kept(n, tree0, ab, bytes(cl.result(0)), bytes(cl.result(1)))
        assert outs.collect() == want[fused][:4], ("buffers", fused)
        outs.free()
        # two views of one allocation: the tree in its first n words, the leaves in the n behind them
        outs = _Outs(m, 950 + m)
        tree, a = both.view(0, 32 * n), both.view(32 * n, 32 * n)
        both.upload(fill(n, 6) + ab)
        cl.mle_tree(tree, a)
        cl.wait_result()
        before = bytes(both.download())
        cl.gkr_prove(tree, a, outs.state, weight=outs.weight, rounds=outs.rounds, points=outs.points, claims=outs.claims, fused=fused)
        cl.wait_result()
        after = bytes(both.download())
        _kept(n, before[:32 * n], ab, after[:32 * n], after[32 * n:])
        assert outs.collect() == want[fused][:4], ("views", fused)
        outs.free()
    both.free()
    cl.close()


def test_refusals_and_the_order_of_checks(gpu):
    """Every refusal returns BLZ_ERR_INVALID_PARAM with its own message, leaves nothing in flight and changes no byte; a call wrong
    in two ways reports the earlier check; the good call behind them all equals the prover on Python integers."""
    field, m = "BLS381", 4
    n = 1 << m
    lay = gkr.layout(m)
    leaves = _leaves(field, m)
    ab = _pack(leaves)
    cl = _client(field, m)
    L = blaze_amd.lib()
    a, tree = _dev(ab), _dev(fill(n, 1))
    cl.mle_tree(tree, a)
    cl.wait_result()
    tb = bytes(tree.download())
    cl.set_data(NTTInput(0, tb)); cl.set_data(NTTInput(1, ab))
    outs_b = fill(64, 2)[:32] + STATE0 + fill(64, 2)[64:]
    outs, weight = _dev(outs_b), _dev(fill(8, 3))   # the state at word 1, rounds at 4 (18 words), points at 24 (10), claims at 36 (8)
    st, ro, po, c0 = outs.ptr + 32, outs.ptr + 32 * 4, outs.ptr + 32 * 24, outs.ptr + 32 * 36
    assert (lay.rounds_words, lay.points_words, lay.claims_words, lay.weight_words) == (18, 10, 8, 4)
    wb = bytes(weight.download())
    host = (C.c_char * 64)()
    host_ptr = C.addressof(host)

    def gk(op=PROD, flags=0, t=tree, x=a, length=n, w=weight.ptr, s=st, rd=ro, p=po, c=c0):
        return lambda: raw_gkr(cl, op, flags, t, x, length, w, s, rd, p, c)

    refused = [
        (lambda: L.blz_ntt_gkr_prove(None, 0, 0, None, None, 0, None, None, None, None, None), "null handle"),
        (gk(op=FRAC), "BLZ_TREE_FRAC is not built"), (gk(op=7), "unknown tree op 7"), (gk(flags=2), "unknown GKR flags 0x2"), (gk(flags=0x80000001), "unknown GKR flags"),
        (gk(t=None), "tree is NULL"), (gk(x=None), "a is NULL"), (gk(w=None), "d_weight is NULL"), (gk(s=None), "d_state is NULL"),
        (gk(rd=None), "d_rounds is NULL"), (gk(p=None), "d_points is NULL"), (gk(c=None), "d_claims is NULL"),
        (gk(length=1), "len 1:"), (gk(length=12), "len 12:"), (gk(length=2 * n), f"len {2 * n}:"),
        (gk(t=BlzVecArg(tree.ptr, 0, 0, 3)), "operand tree: count 3 is not a power of two"), (gk(x=BlzVecArg(None, 2, 0, 0)), "operand a: buf must be 0 or 1"),
        (gk(t=tree.view(0, 32 * 8)), "operand tree: 8 words, a tree over len 16 holds len - 1"),
        (gk(x=a.view(0, 32 * 8)), "operand a: 8 words, read periodically over len 16"),
        (gk(w=weight.ptr + 8), "d_weight: the pointer is not 16-byte aligned"), (gk(s=host_ptr), "d_state: the pointer is not"),
        (gk(rd=outs.ptr + 32 * 50), "d_rounds: 18 elements run past the end"), (gk(p=outs.ptr + 32 * 60), "d_points: 10 elements run past the end"),
        (gk(c=outs.ptr + 32 * 57), "d_claims: 8 elements run past the end"), (gk(w=weight.ptr + 32 * 5), "d_weight: 4 elements run past the end"),
        (gk(x=BlzVecArg(tree.ptr + 32 * 8, 0, 0, 16)), "operand a: 16 elements run past the end"),
        (gk(x=BlzVecArg(tree.ptr, 0, 0, 16)), "a overlaps tree"),
        (gk(w=tree.ptr + 32 * 12), "d_weight overlaps tree"), (gk(w=a.ptr + 32 * 12), "d_weight overlaps a"),
        (gk(s=tree.ptr), "d_state overlaps tree"), (gk(s=a.ptr + 32 * 15), "d_state overlaps a"), (gk(s=weight.ptr + 32 * 3), "d_state overlaps d_weight"),
        (gk(rd=st), "d_rounds overlaps d_state"), (gk(p=ro + 32 * 17), "d_points overlaps d_rounds"), (gk(c=po + 32 * 9), "d_claims overlaps d_points"),
        (gk(c=st), "d_claims overlaps d_state"),
    ]
    # wrong in two ways: the earlier check speaks
    refused += [
        (gk(op=FRAC, flags=2), "BLZ_TREE_FRAC is not built"), (gk(op=9, flags=2), "unknown tree op 9"), (gk(flags=2, t=None), "unknown GKR flags"),
        (gk(t=None, length=12), "tree is NULL"), (gk(c=None, length=12), "d_claims is NULL"), (gk(length=12, w=weight.ptr + 8), "len 12:"),
        (gk(t=tree.view(0, 32 * 8), s=st + 8), "operand tree: 8 words"), (gk(x=a.view(0, 32 * 8), s=st + 8), "operand a: 8 words"),
        (gk(c=c0 + 8, s=tree.ptr), "d_claims: the pointer is not 16-byte aligned"), (gk(x=BlzVecArg(tree.ptr, 0, 0, 16), p=ro), "a overlaps tree"),
        (gk(w=tree.ptr, c=po), "d_weight overlaps tree"), (gk(s=weight.ptr, c=po), "d_state overlaps d_weight"),
    ]

    def unchanged():
        with pytest.raises(DriverClientError) as ei:
            cl.wait_result()   # nothing is in flight
        assert ei.value.variant == "InvalidPrimitiveParam"
        assert bytes(cl.result(0)) == tb and bytes(cl.result(1)) == ab
        assert bytes(tree.download()) == tb and bytes(a.download()) == ab and bytes(weight.download()) == wb and bytes(outs.download()) == outs_b

    for attempt, message in refused:
        assert attempt() == 4, message
        assert message in _err(), (message, _err())
        unchanged()
    # an op already in flight: refused behind the argument checks and the live length, ahead of the operands'
    for attempt, message in ((gk(), "already running"), (gk(flags=2), "unknown GKR flags"), (gk(length=12), "len 12:"),
                             (gk(t=tree.view(0, 32 * 8)), "already running"), (gk(s=st + 8), "already running")):
        cl.vec_mle_round(a)
        assert attempt() == 4 and message in _err(), (message, _err())
        cl.wait_result()
        unchanged()
    # and the good calls behind them all: device words, then the two buffers (the tree in buffer 0)
    root, rounds, points, claims, state = prove_ref(field, leaves, STATE0)
    want = outs_b[:32] + state + outs_b[64:128] + _pack(rounds) + outs_b[32 * 22:32 * 24] + _pack(points) + outs_b[32 * 34:32 * 36] + _pack(claims) + outs_b[32 * 44:]
    for flags, t, x in ((0, tree, a), (UNFUSED, 0, 1)):
        outs.upload(outs_b)
        assert gk(flags=flags, t=t, x=x)() == 0, _err()
        cl.wait_result()
        assert bytes(outs.download()) == want, flags
    assert int.from_bytes(tb[32 * (n - 2):32 * (n - 1)], "little") == root
    cl.close()
    for d in (a, tree, outs, weight):
        d.free()


def test_in_flight_rules(gpu):
    """While the op runs over BOTH transform buffers neither can be read, written or exchanged and no op starts - both count as
    written, on either path; reset drops it, and the handle works afterwards."""
    field, m = "BLS381", 8
    n = 1 << m
    leaves = _leaves(field, m)
    ab = _pack(leaves)
    cl = _client(field, m)
    words, d_state = _dev(ab), _dev(STATE0)
    host_out = bytearray(32 * n)
    root, rounds, points, claims, state = prove_ref(field, leaves, STATE0)
    want = (_pack(rounds), _pack(points), _pack(claims), state)

    def load(tree_buf):
        cl.set_data(NTTInput(1 - tree_buf, ab))
        cl.mle_tree(tree_buf, 1 - tree_buf)
        cl.wait_result()
        d_state.upload(STATE0)

    busy = (lambda: cl.start_process(0), lambda: cl.vec_op(NTTClient.MUL, 1, 1, words), lambda: cl.vec_reduce(NTTClient.FOLD_SUM, 0), lambda: cl.vec_mle_round(words),
            lambda: cl.fs_challenge(d_state, words, count=1), lambda: cl.mle_tree(0, words), lambda: cl.gkr_prove(0, 1, d_state),
            lambda: cl.result(0), lambda: cl.result(1), lambda: cl.set_data(NTTInput(0, ab)), lambda: cl.set_data(NTTInput(1, ab)),
            lambda: cl.exchange(0, ab, host_out), lambda: cl.exchange(1, ab, host_out))
    for tree_buf, fused in ((0, True), (1, True), (0, False)):
        load(tree_buf)
        out = cl.gkr_prove(tree_buf, 1 - tree_buf, d_state, fused=fused)
        for attempt in busy:
            with pytest.raises(DriverClientError) as ei:
                attempt()
            assert ei.value.variant == "InvalidPrimitiveParam"
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        assert tuple(bytes(d.download()) for d in out) + (bytes(d_state.download()),) == want, (tree_buf, fused)
        cl.result(0); cl.result(1)
        for d in out:
            d.free()
    # reset with the op in flight: nothing is in flight afterwards, and the handle works
    load(0)
    out = cl.gkr_prove(0, 1, d_state)
    cl.reset()
    with pytest.raises(DriverClientError):
        cl.wait_result()
    load(0)
    cl.gkr_prove(0, 1, d_state, rounds=out[0], points=out[1], claims=out[2])
    cl.wait_result()
    assert tuple(bytes(d.download()) for d in out) + (bytes(d_state.download()),) == want
    cl.close()
    for d in (words, d_state) + tuple(out):
        d.free()
