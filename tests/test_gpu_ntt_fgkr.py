"""The one-call fraction GKR prover (blz_ntt_gkr_prove_frac, logUp-GKR) on the device.  The trees are built by mle_tree(TREE_FRAC)
in the test.  The fused path - k_fgkr_tail, one block that keeps a layer's four tables in LDS - against the chain of existing
launches (BLZ_GKR_UNFUSED), byte for byte on d_rounds, d_points, d_claims, d_lambdas and d_state; the chain against the
host-driven loop of the single ops; both against the prover on Python integers with edge words among the leaves; the verifier of
blaze_amd/gkr.py on the device output; a logUp instance; the bytes that may and may not change; every refusal in the documented
order; the in-flight rules.  Every run carries guard words on both sides of the five outputs and of the weight, keeps word 0 of
d_lambdas, and checks the parts of the trees and of the leaves that keep their bytes."""
import ctypes as C

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError, fiat_shamir, gkr
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import NTTClient, NTTInput
from ntt_fgkr_util import logup_instance, prove_ref, raw_fgkr
from ntt_gkr_util import mle_at
from ntt_mle_util import fill
from ntt_prove_util import host_loop
from ntt_vec_util import FIELDS, TOP, _client, _dev, _pack, _unpack, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
FRAC, UNFUSED = NTTClient.TREE_FRAC, NTTClient.GKR_UNFUSED
STATE0 = bytes(range(61, 93))
G = 32   # one guard word
TAIL_LOG = 8   # FGKR_TAIL_LOG: the fused path takes the layers of 2^8 words a table and below whole
GATE = [(1, [0, 3]), (1, [2, 1])]   # P_lo Q_hi + Q_lo T over [P_lo, T, Q_lo, Q_hi]


def _err():
    return blaze_amd.lib().blz_last_error_message().decode()


def _leaves(field, m, edges=False):
    """(a_p, a_q): random 256-bit words, more than half of them above the modulus; edges: 0, 1, r - 1, r, r + 1 and 2^256 - 1 among
    the numerators and, at other places, among the denominators"""
    r = pyref.CURVES[field]["r"]
    a_p, a_q = _words(53000 + 10 * m + len(field), 1 << m), _words(54000 + 10 * m + len(field), 1 << m)
    if edges:
        for i, e in enumerate([0, 1, r - 1, r, r + 1, TOP]):
            a_p[(5 * i + 1) % len(a_p)] = e   # 5 and 3 are odd: six distinct places among sixteen
            a_q[(3 * i + 2) % len(a_q)] = e
    return a_p, a_q


def _halves(n, j):
    """(the layer is the leaves, word of lo, word of hi, words of each) of layer j's tables in a tree / the leaves"""
    m = n.bit_length() - 1
    k = m - 1 - j
    off = 0 if k == 0 else NTTClient.tree_layer(n, k)[0]
    return k == 0, off, off + (1 << j), 1 << j


def _kept(n, fused, before, after):
    """before, after: (tree_p, tree_q, a_p, a_q) bytes.  Of tree_p / a_p only the whole hi half and the first half of the lo half
    of a layer may change, of tree_q / a_q only the first half of each half; the root and everything behind it keep their
    bytes; the fused path leaves the layers it takes whole untouched."""
    m = n.bit_length() - 1
    for j in range(m):
        leaf, lo, hi, h = _halves(n, j)
        for which in (0, 1):
            b, a = (before[which + 2], after[which + 2]) if leaf else (before[which], after[which])
            assert a[32 * (lo + h // 2):32 * (lo + h)] == b[32 * (lo + h // 2):32 * (lo + h)], ("upper half of lo", which, j)
            if which == 1:
                assert a[32 * (hi + h // 2):32 * (hi + h)] == b[32 * (hi + h // 2):32 * (hi + h)], ("upper half of Q_hi", j)
            if fused and j <= TAIL_LOG:
                assert a[32 * lo:32 * (hi + h)] == b[32 * lo:32 * (hi + h)], ("a layer the block takes whole", which, j)
    for which in (0, 1):
        assert after[which][32 * (n - 2):] == before[which][32 * (n - 2):], "the root and the word behind it"
    assert [len(x) for x in after] == [len(x) for x in before]


class _Outs:
    """The five outputs and the weight, each between two guard words of random bytes, in two allocations"""

    def __init__(self, m, seed, state0=STATE0):
        self.lay = lay = gkr.layout_frac(m)
        sizes = (1, lay.rounds_words, lay.points_words, lay.claims_words, lay.lambdas_words)
        self.at, pos = [], 1
        for s in sizes:
            self.at.append(pos)
            pos += s + 1
        self.sizes = sizes
        self.fill, self.wfill = fill(pos, seed), fill(lay.weight_words + 2, seed + 1)
        self.fill = self.fill[:G] + state0 + self.fill[2 * G:]   # the transcript starts from state0
        self.buf, self.wbuf = _dev(self.fill), _dev(self.wfill)
        self.state, self.rounds, self.points, self.claims, self.lambdas = (self.buf.view(32 * a, 32 * s) for a, s in zip(self.at, sizes))
        self.weight = self.wbuf.view(G, 32 * lay.weight_words)

    def kw(self):
        return dict(weight=self.weight, rounds=self.rounds, points=self.points, claims=self.claims, lambdas=self.lambdas)

    def collect(self):
        """(state, rounds, points, claims, lambdas) bytes; the guard words and word 0 of the lambdas are checked on the way"""
        got, wgot = bytes(self.buf.download()), bytes(self.wbuf.download())
        want = bytearray(self.fill)
        out = []
        for a, s in zip(self.at, self.sizes):
            out.append(got[32 * a:32 * (a + s)])
            want[32 * a:32 * (a + s)] = out[-1]
        assert got == bytes(want), "a byte outside the five outputs changed"
        la = self.at[4]
        assert out[4][:32] == self.fill[32 * la:32 * (la + 1)], "word 0 of d_lambdas changed"
        assert wgot[:G] == self.wfill[:G] and wgot[-G:] == self.wfill[-G:], "a guard word of the weight changed"
        return tuple(out)

    def free(self):
        self.buf.free()
        self.wbuf.free()


def _build(cl, ab_p, ab_q, n, seed):
    """(tree_p, tree_q, a_p, a_q) DeviceBuffers with the trees built, and their bytes"""
    a_p, a_q, tree_p, tree_q = _dev(ab_p), _dev(ab_q), _dev(fill(n, seed)), _dev(fill(n, seed + 1))
    cl.mle_tree(tree_p, a_p, FRAC, dst_q=tree_q, a_q=a_q)
    cl.wait_result()
    ops = (tree_p, tree_q, a_p, a_q)
    return ops, tuple(bytes(d.download()) for d in ops)


_RUNS = {}


def _run(field, m, fused, edges=False, leaves=None, key=None):
    """One proof over device words, computed once: (state, rounds, points, claims, lambdas with word 0 cut, root_p, root_q)"""
    key = (field, m, fused, edges, key)
    if key not in _RUNS:
        n = 1 << m
        lp, lq = leaves if leaves is not None else _leaves(field, m, edges)
        cl = _client(field, m)
        ops, before = _build(cl, _pack(lp), _pack(lq), n, 70 + m)
        outs = _Outs(m, 700 + m)
        cl.gkr_prove_frac(*ops, outs.state, **outs.kw(), fused=fused)
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        _kept(n, fused, before, tuple(bytes(d.download()) for d in ops))
        got = outs.collect()
        roots = tuple(int.from_bytes(before[w][32 * (n - 2):32 * (n - 1)], "little") for w in (0, 1))
        _RUNS[key] = got[:4] + (got[4][32:],) + roots
        cl.close()
        for d in ops:
            d.free()
        outs.free()
    return _RUNS[key]


def _want(field, lp, lq):
    """_run's tuple by the prover on Python integers"""
    root_p, root_q, rounds, points, claims, lambdas, state = prove_ref(field, lp, lq, STATE0)
    return (state, _pack(rounds), _pack(points), _pack(claims), _pack(lambdas[1:]), root_p, root_q)


# all-fused up to m = 9, one chain step at the layer of 512, two and three at m = 11 and 12
SIZES = [("BLS381", m) for m in (1, 2, 3, 8, 9, 10, 11, 12)] + [(f, m) for f in ("BLS377", "BN254") for m in (3, 10)]


@pytest.mark.parametrize("field,m", SIZES)
def test_fused_equals_unfused_byte_for_byte(gpu, field, m):
    one, chain = _run(field, m, True), _run(field, m, False)
    for what, x, y in zip(("d_state", "d_rounds", "d_points", "d_claims", "d_lambdas", "root_p", "root_q"), one, chain):
        assert x == y, what
    assert one[0] != STATE0
    r = pyref.CURVES[field]["r"]
    assert all(v < r for part in one[1:5] for v in _unpack(part)) or m == 1   # canonical; at m = 1 the claims are the leaves as stored


def _host_driven(cl, field, n, ops, state):
    """The proof by the single ops with the host between them: per layer fs_challenge with count 0, gate_eval for T in place,
    vec_mle_eq, ntt_prove_util.host_loop over views of the layer, a download of the four final words, hashlib.  Returns
    (state, rounds, points, claims, lambdas from word 1) bytes."""
    r = pyref.CURVES[field]["r"]
    m = n.bit_length() - 1
    tree_p, tree_q, a_p, a_q = ops
    eq, d_state, d_lam = DeviceBuffer(0, 32 * max(n // 4, 1)), _dev(state), DeviceBuffer(0, 32)
    rounds, points, claims, lambdas, tau = b"", [], b"", b"", []
    for j in range(m):
        leaf, lo, hi, h = _halves(n, j)
        bp, bq = (a_p, a_q) if leaf else (tree_p, tree_q)
        plo, phi, qlo, qhi = bp.view(32 * lo, 32 * h), bp.view(32 * hi, 32 * h), bq.view(32 * lo, 32 * h), bq.view(32 * hi, 32 * h)
        z = []
        if j >= 1:
            d_state.upload(state)
            cl.fs_challenge(d_state, None, 0, r=d_lam)
            cl.wait_result()
            state, lam = fiat_shamir.absorb(state, [], field)
            assert bytes(d_state.download()) == state and bytes(d_lam.download()) == _pack([lam])
            lambdas += _pack([lam])
            cl.gate_eval(phi, [phi, d_lam, qhi], [(1, [0]), (1, [1, 2])], length=h)   # T over P_hi
            cl.wait_result()
            point = _dev(_pack(tau))
            cl.vec_mle_eq(eq, point, j - 1)
            cl.wait_result()
            point.free()
            rows, chal, state, _ = host_loop(cl, field, [plo, phi, qlo, qhi], GATE, None, eq.view(0, 32 * max(h // 2, 1)), 3, h, state)
            rounds += rows
            z = chal[::-1]
            f = [int.from_bytes(bytes(t.download(32)), "little") for t in (plo, phi, qlo, qhi)]
            f[1] = (f[1] - lam * f[3]) % r
            row = _pack(f)
        else:
            row = b"".join(bytes(t.download(32)) for t in (plo, phi, qlo, qhi))
        claims += row
        state, rho = fiat_shamir.absorb(state, row, field)
        tau = z + [rho]
        points += tau
    for d in (eq, d_state, d_lam):
        d.free()
    return state, rounds, _pack(points), claims, lambdas


@pytest.mark.parametrize("m", (1, 2, 6, 10))
def test_unfused_equals_the_host_driven_loop(gpu, m):
    field, n = "BLS381", 1 << m
    lp, lq = _leaves(field, m)
    cl = _client(field, m)
    ops, _ = _build(cl, _pack(lp), _pack(lq), n, 11)
    want = _host_driven(cl, field, n, ops, STATE0)
    assert _run(field, m, False)[:5] == want
    cl.close()
    for d in ops:
        d.free()


@pytest.mark.parametrize("field", FIELDS)
def test_prover_on_python_integers_and_edge_words(gpu, field):
    """m = 4: both paths equal the prover written on Python integers, over random words and over leaves that hold 0, 1, r - 1, r,
    r + 1 and 2^256 - 1 in both tables - which the fused kernel reads as stored."""
    r = pyref.CURVES[field]["r"]
    for edges in (False, True):
        lp, lq = _leaves(field, 4, edges)
        if edges:
            assert all(e in lp and e in lq for e in (0, 1, r - 1, r, r + 1, TOP))
        want = _want(field, lp, lq)
        assert _run(field, 4, True, edges) == want, ("fused", edges)
        assert _run(field, 4, False, edges) == want, ("unfused", edges)
    # m = 1: the claims are the four leaves as stored, above the modulus or not
    lp, lq = [TOP, r + 1], [r, TOP - 1]
    want = _want(field, lp, lq)
    assert want[3] == _pack([lp[0], lp[1], lq[0], lq[1]]) and want[1] == b"" and want[4] == b""
    for fused in (True, False):
        assert _run(field, 1, fused, leaves=(lp, lq), key="as stored") == want, fused


@pytest.mark.parametrize("m", (4, 9, 11))
def test_verifier_accepts_the_device_output(gpu, m):
    field = "BLS381"
    r = pyref.CURVES[field]["r"]
    lp, lq = _leaves(field, m)
    state, rounds, points, claims, lambdas, root_p, root_q = _run(field, m, True)
    want = sum(p * pow(q, -1, r) for p, q in zip(lp, lq)) % r
    assert root_p * pow(root_q, -1, r) % r == want
    lambdas = bytes(32) + lambdas
    final, point, (claim_p, claim_q) = gkr.verify_fraction(field, m, root_p, root_q, STATE0, rounds, points, claims, lambdas)
    assert final == state and len(point) == m
    assert claim_p == mle_at(lp, point, r) and claim_q == mle_at(lq, point, r)
    with pytest.raises(ValueError, match="layer 0"):
        gkr.verify_fraction(field, m, (root_p + 1) % r, root_q, STATE0, rounds, points, claims, lambdas)
    with pytest.raises(ValueError, match="layer 0"):
        gkr.verify_fraction(field, m, root_p, (root_q + 1) % r, STATE0, rounds, points, claims, lambdas)


@pytest.mark.parametrize("fused", (True, False))
def test_logup_instance_is_proved_and_verified(gpu, fused):
    """2^5 lookups into a table of 2^5 values, 64 fractions: the root numerator is 0, the proof verifies from the outputs alone;
    with one corrupted lookup the numerator is not 0 (and that proof verifies too: it proves the sum, whatever it is)."""
    field = "BLS381"
    r = pyref.CURVES[field]["r"]
    for bad in (False, True):
        lp, lq = logup_instance(field, bad=bad)
        got = _run(field, 6, fused, leaves=(lp, lq), key=("logup", bad))
        assert got == _want(field, lp, lq)
        state, rounds, points, claims, lambdas, root_p, root_q = got
        assert (root_p == 0) == (not bad) and root_q != 0
        final, point, (claim_p, claim_q) = gkr.verify_fraction(field, 6, root_p, root_q, STATE0, rounds, points, claims, bytes(32) + lambdas)
        assert final == state and claim_p == mle_at(lp, point, r) and claim_q == mle_at(lq, point, r)


@pytest.mark.parametrize("m", (5, 10))
def test_bytes_buffers_and_views(gpu, m):
    """Guard words, word 0 of d_lambdas and the kept parts are checked by every run (m = 5 and 10, both paths, here).  The same
    proof with the two trees as the handle's two transform buffers, and with the four operands as views of one allocation."""
    field, n = "BLS381", 1 << m
    lp, lq = _leaves(field, m)
    abp, abq = _pack(lp), _pack(lq)
    want = {fused: _run(field, m, fused) for fused in (True, False)}
    assert want[True] == want[False]
    cl = _client(field, m)
    both = DeviceBuffer(0, 4 * 32 * n)
    a_p, a_q = _dev(abp), _dev(abq)
    for fused in (True, False):
        # the handle's two buffers: tree_p in buffer 0, tree_q in buffer 1, the leaves device words
        outs = _Outs(m, 900 + m)
        a_p.upload(abp); a_q.upload(abq)
        cl.set_data(NTTInput(0, fill(n, 5))); cl.set_data(NTTInput(1, fill(n, 6)))
        cl.mle_tree(0, a_p, FRAC, dst_q=1, a_q=a_q)
        cl.wait_result()
        before = (bytes(cl.result(0)), bytes(cl.result(1)), abp, abq)
        cl.gkr_prove_frac(0, 1, a_p, a_q, outs.state, **outs.kw(), fused=fused)
        cl.wait_result()
        _kept(n, fused, before, (bytes(cl.result(0)), bytes(cl.result(1)), bytes(a_p.download()), bytes(a_q.download())))
        got = outs.collect()
        assert got[:4] + (got[4][32:],) == want[fused][:5], ("buffers", fused)
        outs.free()
        # four views of one allocation: tree_p, tree_q, a_p, a_q, n words each
        outs = _Outs(m, 950 + m)
        views = tuple(both.view(32 * n * k, 32 * n) for k in range(4))
        both.upload(fill(2 * n, 7) + abp + abq)
        cl.mle_tree(views[0], views[2], FRAC, dst_q=views[1], a_q=views[3])
        cl.wait_result()
        raw = bytes(both.download())
        before = tuple(raw[32 * n * k:32 * n * (k + 1)] for k in range(4))
        cl.gkr_prove_frac(*views, outs.state, **outs.kw(), fused=fused)
        cl.wait_result()
        raw = bytes(both.download())
        _kept(n, fused, before, tuple(raw[32 * n * k:32 * n * (k + 1)] for k in range(4)))
        got = outs.collect()
        assert got[:4] + (got[4][32:],) == want[fused][:5], ("views", fused)
        outs.free()
    for d in (both, a_p, a_q):
        d.free()
    cl.close()


def test_refusals_and_the_order_of_checks(gpu):
    """Every refusal returns BLZ_ERR_INVALID_PARAM with its own message, leaves nothing in flight and changes no byte; a call wrong
    in two ways reports the earlier check; the good call behind them all equals the prover on Python integers."""
    field, m = "BLS381", 4
    n = 1 << m
    lay = gkr.layout_frac(m)
    lp, lq = _leaves(field, m)
    cl = _client(field, m)
    L = blaze_amd.lib()
    (tp, tq, ap, aq), before = _build(cl, _pack(lp), _pack(lq), n, 1)
    cl.set_data(NTTInput(0, before[0])); cl.set_data(NTTInput(1, before[1]))
    outs_b = fill(64, 2)[:32] + STATE0 + fill(64, 2)[64:]
    # the state at word 1, rounds at 4 (18 words), points at 24 (10), claims at 36 (16), lambdas at 54 (4)
    outs, weight = _dev(outs_b), _dev(fill(8, 3))
    st, ro, po, c0, la = (outs.ptr + 32 * k for k in (1, 4, 24, 36, 54))
    assert (lay.rounds_words, lay.points_words, lay.claims_words, lay.lambdas_words, lay.weight_words) == (18, 10, 16, 4, 4)
    wb = bytes(weight.download())
    host = (C.c_char * 64)()
    host_ptr = C.addressof(host)

    def gk(flags=0, p=tp, q=tq, x=ap, y=aq, length=n, w=weight.ptr, s=st, rd=ro, pt=po, c=c0, lm=la):
        return lambda: raw_fgkr(cl, flags, p, q, x, y, length, w, s, rd, pt, c, lm)

    refused = [
        (lambda: L.blz_ntt_gkr_prove_frac(None, 0, None, None, None, None, 0, None, None, None, None, None, None), "null handle"),
        (gk(flags=2), "unknown GKR flags 0x2"), (gk(flags=0x80000001), "unknown GKR flags"),
        (gk(p=None), "tree_p is NULL"), (gk(q=None), "tree_q is NULL"), (gk(x=None), "a_p is NULL"), (gk(y=None), "a_q is NULL"), (gk(w=None), "d_weight is NULL"),
        (gk(s=None), "d_state is NULL"), (gk(rd=None), "d_rounds is NULL"), (gk(pt=None), "d_points is NULL"), (gk(c=None), "d_claims is NULL"),
        (gk(lm=None), "d_lambdas is NULL"),
        (gk(length=1), "len 1:"), (gk(length=12), "len 12:"), (gk(length=2 * n), f"len {2 * n}:"),
        (gk(p=BlzVecArg(tp.ptr, 0, 0, 3)), "operand tree_p: count 3 is not a power of two"), (gk(q=BlzVecArg(None, 2, 0, 0)), "operand tree_q: buf must be 0 or 1"),
        (gk(x=BlzVecArg(ap.ptr, 0, 1, 16)), "operand a_p: reserved must be 0"), (gk(y=BlzVecArg(aq.ptr + 32 * 8, 0, 0, 16)), "operand a_q: 16 elements run past the end"),
        (gk(p=tp.view(0, 32 * 8)), "operand tree_p: 8 words, a tree over len 16 holds len - 1"),
        (gk(q=tq.view(0, 32 * 8)), "operand tree_q: 8 words, a tree over len 16 holds len - 1"),
        (gk(x=ap.view(0, 32 * 8)), "operand a_p: 8 words, read periodically over len 16"),
        (gk(y=aq.view(0, 32 * 8)), "operand a_q: 8 words, read periodically over len 16"),
        (gk(w=weight.ptr + 8), "d_weight: the pointer is not 16-byte aligned"), (gk(s=host_ptr), "d_state: the pointer is not"),
        (gk(rd=outs.ptr + 32 * 50), "d_rounds: 18 elements run past the end"), (gk(pt=outs.ptr + 32 * 60), "d_points: 10 elements run past the end"),
        (gk(c=outs.ptr + 32 * 57), "d_claims: 16 elements run past the end"), (gk(lm=outs.ptr + 32 * 62), "d_lambdas: 4 elements run past the end"),
        (gk(w=weight.ptr + 32 * 5), "d_weight: 4 elements run past the end"),
        (gk(q=BlzVecArg(tp.ptr, 0, 0, 16)), "tree_q overlaps tree_p"), (gk(q=0, p=0), "tree_q overlaps tree_p"),
        (gk(x=BlzVecArg(tp.ptr, 0, 0, 16)), "a_p overlaps tree_p"), (gk(y=BlzVecArg(tq.ptr, 0, 0, 16)), "a_q overlaps tree_q"),
        (gk(y=BlzVecArg(ap.ptr, 0, 0, 16)), "a_q overlaps a_p"),
        (gk(w=tp.ptr + 32 * 12), "d_weight overlaps tree_p"), (gk(w=tq.ptr + 32 * 11), "d_weight overlaps tree_q"), (gk(w=ap.ptr + 32 * 12), "d_weight overlaps a_p"),
        (gk(w=aq.ptr + 32 * 12), "d_weight overlaps a_q"),
        (gk(s=tp.ptr), "d_state overlaps tree_p"), (gk(s=aq.ptr + 32 * 15), "d_state overlaps a_q"), (gk(s=weight.ptr + 32 * 3), "d_state overlaps d_weight"),
        (gk(rd=st), "d_rounds overlaps d_state"), (gk(pt=ro + 32 * 17), "d_points overlaps d_rounds"), (gk(c=po + 32 * 9), "d_claims overlaps d_points"),
        (gk(c=outs.ptr), "d_claims overlaps d_state"), (gk(lm=c0 + 32 * 15), "d_lambdas overlaps d_claims"), (gk(lm=st), "d_lambdas overlaps d_state"),
        (gk(lm=tq.ptr + 32 * 12), "d_lambdas overlaps tree_q"),
    ]
    # wrong in two ways: the earlier check speaks
    refused += [
        (gk(flags=2, p=None), "unknown GKR flags"), (gk(p=None, q=None), "tree_p is NULL"), (gk(y=None, length=12), "a_q is NULL"),
        (gk(lm=None, length=12), "d_lambdas is NULL"), (gk(length=12, w=weight.ptr + 8), "len 12:"),
        (gk(p=tp.view(0, 32 * 8), s=st + 8), "operand tree_p: 8 words"), (gk(y=aq.view(0, 32 * 8), s=st + 8), "operand a_q: 8 words"),
        (gk(q=tq.view(0, 32 * 8), x=ap.view(0, 32 * 8)), "operand tree_q: 8 words"),
        (gk(lm=la + 8, s=tp.ptr), "d_lambdas: the pointer is not 16-byte aligned"), (gk(w=weight.ptr + 8, lm=la + 8), "d_weight: the pointer is not"),
        (gk(x=BlzVecArg(tp.ptr, 0, 0, 16), pt=ro), "a_p overlaps tree_p"), (gk(w=tp.ptr, c=po), "d_weight overlaps tree_p"),
        (gk(s=weight.ptr, c=po), "d_state overlaps d_weight"), (gk(c=po, lm=po), "d_claims overlaps d_points"),
    ]

    def unchanged():
        with pytest.raises(DriverClientError) as ei:
            cl.wait_result()   # nothing is in flight
        assert ei.value.variant == "InvalidPrimitiveParam"
        assert bytes(cl.result(0)) == before[0] and bytes(cl.result(1)) == before[1]
        assert tuple(bytes(d.download()) for d in (tp, tq, ap, aq)) == before
        assert bytes(weight.download()) == wb and bytes(outs.download()) == outs_b

    for attempt, message in refused:
        assert attempt() == 4, message
        assert message in _err(), (message, _err())
        unchanged()
    # an op already in flight: refused behind the argument checks and the live length, ahead of the operands'
    for attempt, message in ((gk(), "already running"), (gk(flags=2), "unknown GKR flags"), (gk(length=12), "len 12:"),
                             (gk(p=tp.view(0, 32 * 8)), "already running"), (gk(s=st + 8), "already running")):
        cl.vec_mle_round(ap)
        assert attempt() == 4 and message in _err(), (message, _err())
        cl.wait_result()
        unchanged()
    # and the good calls behind them all: device words, then the trees in the two buffers
    w = _want(field, lp, lq)
    want = (outs_b[:32] + w[0] + outs_b[64:128] + w[1] + outs_b[32 * 22:32 * 24] + w[2] + outs_b[32 * 34:32 * 36] + w[3] + outs_b[32 * 52:32 * 55] + w[4]
            + outs_b[32 * 58:])
    for flags, p, q in ((0, tp, tq), (UNFUSED, 0, 1)):
        outs.upload(outs_b)
        ap.upload(before[2]); aq.upload(before[3])
        assert gk(flags=flags, p=p, q=q)() == 0, _err()
        cl.wait_result()
        assert bytes(outs.download()) == want, flags
    assert tuple(int.from_bytes(before[k][32 * (n - 2):32 * (n - 1)], "little") for k in (0, 1)) == w[5:]
    cl.close()
    for d in (tp, tq, ap, aq, outs, weight):
        d.free()


def test_in_flight_rules(gpu):
    """While the op runs over BOTH transform buffers neither can be read, written or exchanged and no op starts - both count as
    written, on either path; reset drops it, and the handle works afterwards."""
    field, m = "BLS381", 8
    n = 1 << m
    lp, lq = _leaves(field, m)
    abp, abq = _pack(lp), _pack(lq)
    cl = _client(field, m)
    a_p, a_q, d_state = _dev(abp), _dev(abq), _dev(STATE0)
    host_out = bytearray(32 * n)
    w = _want(field, lp, lq)
    lay = gkr.layout_frac(m)

    def load(swap):
        a_p.upload(abp); a_q.upload(abq)
        cl.mle_tree(swap, a_p, FRAC, dst_q=1 - swap, a_q=a_q)
        cl.wait_result()
        d_state.upload(STATE0)

    def collect(out):
        got = tuple(bytes(d.download()) for d in out)
        return (bytes(d_state.download()),) + got[:3] + (got[3][32:],)

    busy = (lambda: cl.start_process(0), lambda: cl.vec_op(NTTClient.MUL, 1, 1, a_p), lambda: cl.vec_reduce(NTTClient.FOLD_SUM, 0), lambda: cl.vec_mle_round(a_p),
            lambda: cl.fs_challenge(d_state, a_p, count=1), lambda: cl.mle_tree(0, a_p), lambda: cl.gkr_prove_frac(0, 1, a_p, a_q, d_state),
            lambda: cl.result(0), lambda: cl.result(1), lambda: cl.set_data(NTTInput(0, abp)), lambda: cl.set_data(NTTInput(1, abp)),
            lambda: cl.exchange(0, abp, host_out), lambda: cl.exchange(1, abp, host_out))
    for swap, fused in ((0, True), (1, True), (0, False)):
        load(swap)
        out = cl.gkr_prove_frac(swap, 1 - swap, a_p, a_q, d_state, fused=fused)
        assert [d.nbytes for d in out] == [32 * k for k in (lay.rounds_words, lay.points_words, lay.claims_words, lay.lambdas_words)]
        for attempt in busy:
            with pytest.raises(DriverClientError) as ei:
                attempt()
            assert ei.value.variant == "InvalidPrimitiveParam"
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        assert collect(out) == w[:5], (swap, fused)
        cl.result(0); cl.result(1)
        for d in out:
            d.free()
    # reset with the op in flight: nothing is in flight afterwards, and the handle works
    load(0)
    out = cl.gkr_prove_frac(0, 1, a_p, a_q, d_state)
    cl.reset()
    with pytest.raises(DriverClientError):
        cl.wait_result()
    load(0)
    cl.gkr_prove_frac(0, 1, a_p, a_q, d_state, rounds=out[0], points=out[1], claims=out[2], lambdas=out[3])
    cl.wait_result()
    assert collect(out) == w[:5]
    cl.close()
    for d in (a_p, a_q, d_state) + tuple(out):
        d.free()
