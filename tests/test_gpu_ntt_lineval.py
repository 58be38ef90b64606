"""Gate evaluation with linear-form factors (blz_ntt_gate_eval_lin) on the device: products of sums given as data, evaluated at
every position, with periodic tables, rotations and in place; agreement with blz_ntt_gate_eval where the two overlap; the
refusals and the in-flight rules.  Every expected value is Python integer arithmetic (tests/ntt_lin_util.py: lin_value / lin_ref
over gate_inputs) or, at 2^20, the existing op, and every comparison is byte for byte: any 256-bit input word counts as its
residue, every word written is canonical, exactly len words of dst are written and no other byte - of dst, of a table, of the
other buffer - changes."""
import ctypes as C
import itertools
import random

import pytest

import blaze_amd
from blaze_amd import DeviceBuffer, DriverClientError
from blaze_amd._lib import BlzVecArg
from blaze_amd.ingo_ntt import FORM, NTTClient, NTTInput
from ntt_gate_util import CATALOGUE as SUM_CATALOGUE, gate_inputs
from ntt_lin_util import CATALOGUE, PERM_FORMS, PERM_ROT, PERM_TERMS, lin_ref, make_lin_gate, perm_counts, raw_lin
from ntt_mle_util import fill
from ntt_spmv_util import _inputs
from ntt_vec_util import FIELDS, TOP, _client, _dev, _pack, _words
from oracle import pyref

pytestmark = pytest.mark.gpu
# (log n, len), test_gpu_ntt_gate_eval.py's: a single word and a ragged tail put lanes and whole blocks at or above len in front
# of the kernel's barrier
SIZES = [(1, 2), (2, 1), (6, 64), (10, 1024), (10, 777), (11, 2048)]
M64 = (1 << 64) - 1


def _bytes_of(cl, t):
    return bytes(t.download()) if isinstance(t, DeviceBuffer) else bytes(cl.result(t))


def _free(items):
    for d in {id(x): x for x in items if isinstance(x, DeviceBuffer)}.values():
        d.free()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn,length", SIZES)
def test_without_forms_it_is_gate_eval(gpu, field, logn, length):
    """nforms = 0: every gate of ntt_gate_util.CATALOGUE through the new op gives gate_eval's bytes and the integers."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    out, out2 = _dev(fill(n, 7)), _dev(fill(n, 7))
    for turn, (name, (nt, terms, common)) in enumerate(SUM_CATALOGUE.items()):
        vals = gate_inputs(r, nt, n, 21000 * logn + 100 * turn + len(field))
        tabs = [_dev(_pack(v)) for v in vals]
        cl.set_data(NTTInput(0, _pack(vals[0])))
        tabs[0].free()
        tabs[0] = 0
        cl.gate_eval(out, tabs, terms, common, length=length)
        cl.wait_result()
        cl.gate_eval_lin(out2, tabs, [], terms, common, length=length)
        cl.wait_result()
        got = bytes(out2.download())
        assert got == bytes(out.download()), name
        assert got == _pack(lin_ref(vals, [], terms, common, r, length)) + fill(n, 7)[32 * length:], name
        _free(tabs)
    cl.close()
    _free([out, out2])


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("logn,length", SIZES)
def test_catalogue_against_python_integers(gpu, field, logn, length):
    """Every form gate of the catalogue.  One n-word table sits in transform buffer 0 - which one moves with the gate -, the rest
    in device words; dst is device words on even turns and transform buffer 1 on odd ones.  Exactly len words of dst are
    written; no other byte of dst, of a table or of the other buffer changes."""
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    out = DeviceBuffer(0, 32 * n)
    for turn, (name, (nt, forms, terms, common, counts, rot, same)) in enumerate(CATALOGUE.items()):
        vals = [v[:k] for v, k in zip(gate_inputs(r, nt, n, 31000 * logn + 100 * turn + len(field)), counts(n))]
        for j, i in same.items():
            vals[j] = vals[i]
        raw = [_pack(v) for v in vals]
        whole = [j for j in range(nt) if len(vals[j]) == n and j not in same and j not in same.values()]
        in_buffer = whole[turn % len(whole)]
        held = [raw[in_buffer], fill(n, 2 * turn + 1)]
        tabs = []
        for j, b in enumerate(raw):
            tabs.append(0 if j == in_buffer else tabs[same[j]] if j in same else _dev(b))
        for b in (0, 1):
            cl.set_data(NTTInput(b, held[b]))
        dst = out if turn % 2 == 0 else 1
        before = fill(n, 90 + turn) if dst is out else held[1]
        out.upload(fill(n, 90 + turn))
        want = lin_ref(vals, forms, terms, common, r, length, rot)
        cl.gate_eval_lin(dst, tabs, forms, terms, common, rot=rot, length=length)
        cl.wait_result()
        assert cl.last_kernel_ms() > 0
        assert _bytes_of(cl, dst) == _pack(want) + before[32 * length:], (name, "dst")
        for j, t in enumerate(tabs):
            assert _bytes_of(cl, t) == raw[j], (name, j, "a table changed")
        if dst is out:
            assert bytes(cl.result(1)) == held[1], (name, "the other buffer changed")
        else:
            assert bytes(out.download()) == fill(n, 90 + turn)
        _free(tabs)
    cl.close()
    out.free()


@pytest.mark.parametrize("field", FIELDS)
def test_edge_words_in_every_slot(gpu, field):
    """c0 x0 + c1 x1 with every combination of 0, 1, r - 1, r, r + 1, 2^256 - 1 in the four slots (6^4 positions): once with the
    coefficients as n-word tables, then with the two coefficient slots taken by one-word tables, once per pair of edge values.
    Then a four-factor term of four-summand forms with 2^256 - 1 in every slot, added and negated, under a table and under a
    form as common factor."""
    logn = 11
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    edges = [0, 1, r - 1, r, r + 1, TOP]
    combos = list(itertools.product(edges, repeat=4))
    vals = [[c[j] for c in combos] + _words(500 + j + len(field), n - len(combos)) for j in range(4)]   # c0, x0, c1, x1
    forms, terms = [[(1, 0, 1), (1, 2, 3)]], [(1, [FORM])]
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, _pack(vals[1])))
    tabs = [_dev(_pack(vals[0])), 0, _dev(_pack(vals[2])), _dev(_pack(vals[3]))]
    out = DeviceBuffer(0, 32 * n)
    cl.gate_eval_lin(out, tabs, forms, terms)
    cl.wait_result()
    assert bytes(out.download()) == _pack(lin_ref(vals, forms, terms, None, r, n))
    c0, c1 = DeviceBuffer(0, 32), DeviceBuffer(0, 32)
    for e0, e1 in itertools.product(edges, repeat=2):
        c0.upload(e0.to_bytes(32, "little"))
        c1.upload(e1.to_bytes(32, "little"))
        for sign in (1, -1):
            f2 = [[(sign, 0, 1), (-sign, 2, 3)]]
            cl.gate_eval_lin(out, [c0, 0, c1, tabs[3]], f2, terms, length=len(combos))
            cl.wait_result()
            assert bytes(out.download(32 * len(combos))) == _pack(lin_ref([[e0], vals[1], [e1], vals[3]], f2, terms, None, r, len(combos))), (e0, e1, sign)
    # 2^256 - 1 in every slot of four four-summand forms: tables 0 .. 3 all TOP (n words, 4 words, one word, n words), table 4 random
    tv = [[TOP] * n, [TOP] * 4, [TOP], [TOP] * n, vals[3]]
    tt = [_dev(_pack(v)) for v in tv]
    for sign in (1, -1):
        f4 = [[(sign, 2, 0), (sign, 1, 3), (sign, None, 1), (sign, 0, 0)], [(sign, None, 0)] * 4, [(sign, 2, 2)] * 4, [(-sign, 3, 1), (sign, 2, 3), (sign, 2, 0), (sign, 1, 1)]]
        t4 = [(sign, [FORM, FORM + 1, FORM + 2, FORM + 3]), (-sign, [FORM + 3, FORM + 3, FORM + 3, FORM + 3])]
        for common in (None, 0, 4, FORM + 1, FORM + 3):
            cl.gate_eval_lin(out, tt, f4, t4, common, length=300)
            cl.wait_result()
            assert bytes(out.download(32 * 300)) == _pack(lin_ref(tv, f4, t4, common, r, 300)), (sign, common)
    cl.close()
    _free(tabs + tt + [out, c0, c1])


@pytest.mark.parametrize("field", FIELDS)
def test_periodic_tables_and_rotations(gpu, field):
    """Tables of 1, 4 and n words mixed; a coefficient and its table rotated independently, n - 1 and 2^64 - 1 among the
    rotations; rot = NULL against all zeros; the same words under two indices with two rotations."""
    logn = 9
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    counts = [n, 4, 1, n, n, 4]
    vals = [v[:k] for v, k in zip(gate_inputs(r, 6, n, 33000 + len(field)), counts)]
    cl.set_data(NTTInput(0, _pack(vals[0])))
    tabs = [0] + [_dev(_pack(v)) for v in vals[1:]]
    out = DeviceBuffer(0, 32 * n)
    # (c4 x0 - c1 x3 + c2 x4 + x5) (x3 + c0 x0) - x1
    forms = [[(1, 4, 0), (-1, 1, 3), (1, 2, 4), (1, None, 5)], [(1, None, 3), (1, 0, 0)]]
    terms = [(1, [FORM, FORM + 1]), (-1, [1])]
    cases = [[k] * 6 for k in (0, 1, 4, n - 1, n, M64)]
    cases += [[n - 1, 0, 0, 0, M64, 0], [1, 4, n - 1, 3, M64, 2 * n + 5], [(1 << 63) + 7, M64, 5, n - 1, 1, 2]]
    for rot in cases:
        cl.gate_eval_lin(out, tabs, forms, terms, rot=rot, length=n - 3)
        cl.wait_result()
        assert bytes(out.download())[:32 * (n - 3)] == _pack(lin_ref(vals, forms, terms, None, r, n - 3, rot)), rot
    cl.gate_eval_lin(out, tabs, forms, terms, rot=[-1] * 6)
    cl.wait_result()
    assert bytes(out.download()) == _pack(lin_ref(vals, forms, terms, None, r, n, [M64] * 6))
    # rot = NULL is all zeros
    cl.gate_eval_lin(out, tabs, forms, terms, rot=[0] * 6)
    cl.wait_result()
    zeros = bytes(out.download())
    out.upload(fill(n, 5))
    assert raw_lin(cl, make_lin_gate(6, forms, terms, None), out, tabs, None, n) == 0
    cl.wait_result()
    assert bytes(out.download()) == zeros == _pack(lin_ref(vals, forms, terms, None, r, n))
    # Z(wX) (a + c Z(wX)) - Z (a + c Z): the same words as tables 0 and 1, as factor, as summand and as coefficient's table
    z = tabs[3]
    f2, t2 = [[(1, None, 2), (1, 3, 0)], [(1, None, 2), (1, 3, 1)]], [(1, [0, FORM]), (-1, [1, FORM + 1])]
    zv = [vals[3], vals[3], vals[4], vals[2]]
    cl.gate_eval_lin(out, [z, z, tabs[4], tabs[2]], f2, t2, rot=[1, 0, 0, 0])
    cl.wait_result()
    assert bytes(out.download()) == _pack(lin_ref(zv, f2, t2, None, r, n, [1, 0, 0, 0]))
    cl.close()
    _free(tabs + [out])


@pytest.mark.parametrize("field", FIELDS)
def test_in_place(gpu, field):
    """dst is a table used only inside a form - as a summand's table, as a coefficient - with rotation 0: the out-of-place bytes,
    in device words and in a buffer, over a live length below n.  The three meetings that are refused leave dst as it was."""
    logn = 10
    n = 1 << logn
    length = n - 77
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    vals = gate_inputs(r, 4, n, 34000 + len(field))
    vals[3] = vals[3][:1]
    raw = [_pack(v) for v in vals]
    # (x0 + c3 x1) x2 with dst = table 0 (a summand) or table 1 (a summand under a coefficient); (x2 + c1 x0) with dst = table 1 (a coefficient)
    for forms, terms, place in (([[(1, None, 0), (1, 3, 1)]], [(1, [FORM, 2])], 0), ([[(1, None, 0), (1, 3, 1)]], [(1, [FORM, 2])], 1),
                                ([[(1, None, 2), (-1, 1, 0)]], [(1, [FORM])], 1)):
        want = _pack(lin_ref(vals, forms, terms, None, r, length)) + raw[place][32 * length:]
        devs = [_dev(b) for b in raw]
        cl.gate_eval_lin(devs[place], devs, forms, terms, length=length)   # device words
        cl.wait_result()
        assert bytes(devs[place].download()) == want, place
        cl.set_data(NTTInput(1, raw[place]))
        tabs = devs[:place] + [1] + devs[place + 1:]
        cl.gate_eval_lin(1, tabs, forms, terms, length=length)   # a buffer
        cl.wait_result()
        assert bytes(cl.result(1)) == want, place
        for j, d in enumerate(devs):
            if j != place:
                assert bytes(d.download()) == raw[j], (place, j)
        _free(devs)
    devs = [_dev(b) for b in raw]
    V = BlzVecArg
    forms, terms = [[(1, None, 0), (1, 1, 2)]], [(1, [FORM])]
    g = make_lin_gate(3, forms, terms, None)
    W = [V(d.ptr, 0, 0, n) for d in devs[:3]]
    L = blaze_amd.lib()
    for what, dst, tables, rot, ln, message in (
            ("a coefficient at dst's start, rotated", W[1], W, [0, 1, 0], n, "dst names the words of tables[1], which is rotated by 1"),
            ("a summand at dst's start, rotated", W[2], W, [0, 0, M64], n, "dst names the words of tables[2], which is rotated by"),
            ("a coefficient meeting dst off its start", V(devs[1].ptr + 32 * 4, 0, 0, 8), W, None, 8, "dst overlaps the words of tables[1] without starting where they start"),
            ("a coefficient at dst's start, shorter than len", W[1], [W[0], V(devs[1].ptr, 0, 0, 8), W[2]], None, 9, "dst names the 8 words of tables[1], read periodically over len 9"),
            ("a one-word summand at dst's start", W[2], [W[0], W[1], V(devs[2].ptr, 0, 0, 1)], None, 2, "dst names the 1 words of tables[2], read periodically over len 2")):
        assert raw_lin(cl, g, dst, tables, rot, ln) == 4, what
        assert message in L.blz_last_error_message().decode(), (what, L.blz_last_error_message())
    for j in range(3):
        assert bytes(devs[j].download()) == raw[j]
    # a one-word table may be dst at len 1: gamma <- gamma gamma + x0[0]
    one = _dev(raw[3])
    cl.gate_eval_lin(one, [devs[0], one], [[(1, 1, 1), (1, None, 0)]], [(1, [FORM])], length=1)
    cl.wait_result()
    assert bytes(one.download()) == _pack(lin_ref([vals[0], vals[3]], [[(1, 1, 1), (1, None, 0)]], [(1, [FORM])], None, r, 1))
    cl.close()
    _free(devs + [one])


def test_against_the_existing_ops_at_2_20(gpu):
    """BLS12-381, n = 2^20: two sweeps of the 2048 x 256 grid.  The permutation term in one op gives the bytes of six gate_eval
    calls w + beta sigma + gamma into device words and a seventh over them."""
    field, logn = "BLS381", 20
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    cl = _client(field, logn)
    raw = [random.Random(3400 + j).randbytes(32 * k) for j, k in enumerate(perm_counts(n))]
    raw[1] = raw[0]
    z = _dev(raw[0])
    tabs = [z, z] + [_dev(b) for b in raw[2:]]
    cl.gate_eval_lin(0, tabs, PERM_FORMS, PERM_TERMS, rot=PERM_ROT)
    cl.wait_result()
    tmp = [DeviceBuffer(0, 32 * n) for _ in range(6)]
    for j in range(3):
        cl.gate_eval(tmp[j], [tabs[2 + j], tabs[9], tabs[5 + j], tabs[12]], [(1, [0]), (1, [1, 2]), (1, [3])])
        cl.wait_result()
        cl.gate_eval(tmp[3 + j], [tabs[2 + j], tabs[9 + j], tabs[8], tabs[12]], [(1, [0]), (1, [1, 2]), (1, [3])])
        cl.wait_result()
    cl.gate_eval(1, [z, z] + tmp, [(1, [0, 2, 3, 4]), (-1, [1, 5, 6, 7])], rot=[1] + [0] * 7)
    cl.wait_result()
    got = bytes(cl.result(0))
    assert got == bytes(cl.result(1))
    # and a few positions against Python integers: the first, the last (Z(wX) wraps), the two sides of the second sweep's start
    for p in (0, n - 1, 2048 * 256 - 1, 2048 * 256, 777777):
        v = [int.from_bytes(b[32 * (q % (len(b) // 32)): 32 * (q % (len(b) // 32)) + 32], "little") for b, q in zip(raw, [p + 1] + [p] * 12)]
        assert got[32 * p: 32 * p + 32] == lin_ref([[x] for x in v], PERM_FORMS, PERM_TERMS, None, r, 1)[0].to_bytes(32, "little"), p
    cl.close()
    _free(tabs + tmp)


def test_refusals(gpu):
    """Every description error returns BLZ_ERR_INVALID_PARAM (InvalidPrimitiveParam) with a message that names tables[i], form[k]
    or term[m], and leaves dst, the tables and the in-flight state as they were; the handle then still runs a good call."""
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    L = blaze_amd.lib()
    a, b = _inputs(r, n, 61), _inputs(r, n, 62)
    ab, bb = _pack(a), _pack(b)
    cl = _client(field, logn)
    cl.set_data(NTTInput(0, ab))
    cl.set_data(NTTInput(1, bb))
    words, words2 = _dev(bb), _dev(ab)
    big = _dev(bytes(64 * n))   # 2n words
    host = C.create_string_buffer(32 * n + 64)
    host_ptr = (C.addressof(host) + 63) & ~63
    V = BlzVecArg
    B0, B1, W, W2 = V(None, 0, 0, 0), V(None, 1, 0, n), V(words.ptr, 0, 0, n), V(words2.ptr, 0, 0, n)
    W8 = V(words.ptr, 0, 0, 8)
    FORMS, TERMS = [[(1, 0, 1), (1, None, 0)]], [(1, [FORM, 1])]   # (t0 t1 + t0) t1
    T2 = [B1, W2]

    def ev(gate, dst, tables, rot, length):
        return raw_lin(cl, gate, dst, tables, rot, length)

    def g(nt=2, forms=FORMS, terms=TERMS, common=None):
        return make_lin_gate(nt, forms, terms, common)

    def bent(**fields):
        """the good gate with fields of the description, of its first term, of its first form or of that form's first summand overwritten"""
        x = g()
        for k, v in fields.items():
            if k in ("ntables", "nterms", "common", "nforms"):
                setattr(x, k, v)
            elif k == "term_reserved":
                x.term[0].reserved[v] = 1
            elif k == "form_reserved":
                x.form[0].reserved[v] = 1
            elif k in ("factor0", "factor1"):
                x.term[0].factor[int(k[-1])] = v
            elif k in ("nfactors", "term_negate"):
                setattr(x.term[0], k.replace("term_", ""), v)
            elif k == "nsummands":
                x.form[0].nsummands = v
            else:   # coef, table, negate, reserved of form[0].summand[0]; coef1 / table1 of summand[1]
                setattr(x.form[0].summand[int(k[-1]) if k[-1] == "1" else 0], k.rstrip("1"), v)
        return x

    unused = g(forms=FORMS + [[(1, None, 2)]])   # form[1] is named by no term, and still checked
    assert L.blz_ntt_gate_eval_lin(None, None, None, None, None, 3) == 4 and b"null handle" in L.blz_last_error_message()
    refused = {
        "null gate": (lambda: ev(None, W, T2, None, n), "gate is NULL"),
        "null dst": (lambda: ev(g(), None, T2, None, n), "dst is NULL"),
        "null tables": (lambda: ev(g(), W, None, None, n), "tables is NULL"),
        # the limits
        "ntables 0": (lambda: ev(bent(ntables=0), W, T2, None, n), "ntables 0 is outside [1, 16]"),
        "ntables 17": (lambda: ev(bent(ntables=17), W, [B1] + [W2] * 16, None, n), "ntables 17 is outside [1, 16]"),
        "nterms 0": (lambda: ev(bent(nterms=0), W, T2, None, n), "nterms 0 is outside [1, 8]"),
        "nterms 9": (lambda: ev(bent(nterms=9), W, T2, None, n), "nterms 9 is outside [1, 8]"),
        "nforms 9": (lambda: ev(bent(nforms=9), W, T2, None, n), "nforms 9 is above 8"),
        "nfactors 0": (lambda: ev(bent(nfactors=0), W, T2, None, n), "term[0]: nfactors 0 is outside [1, 4]"),
        "nfactors 5": (lambda: ev(bent(nfactors=5), W, T2, None, n), "term[0]: nfactors 5 is outside [1, 4]"),
        "nsummands 0": (lambda: ev(bent(nsummands=0), W, T2, None, n), "form[0]: nsummands 0 is outside [1, 4]"),
        "nsummands 5": (lambda: ev(bent(nsummands=5), W, T2, None, n), "form[0]: nsummands 5 is outside [1, 4]"),
        # the indices
        "a factor at ntables": (lambda: ev(bent(factor1=2), W, T2, None, n), "term[0]: factor 1 names tables[2], ntables is 2"),
        "a factor of 127": (lambda: ev(bent(factor1=127), W, T2, None, n), "term[0]: factor 1 names tables[127]"),
        "a form at nforms": (lambda: ev(bent(factor0=FORM + 1), W, T2, None, n), "term[0]: factor 0 names form[1], nforms is 1"),
        "a form of 127": (lambda: ev(bent(factor0=255), W, T2, None, n), "term[0]: factor 0 names form[127]"),
        "a form with nforms 0": (lambda: ev(bent(nforms=0), W, T2, None, n), "term[0]: factor 0 names form[0], nforms is 0"),
        "common at ntables": (lambda: ev(bent(common=2), W, T2, None, n), "common 2 is not -1, a table index below ntables 2 or"),
        "common -2": (lambda: ev(bent(common=-2), W, T2, None, n), "common -2 is not -1"),
        "common a form at nforms": (lambda: ev(bent(common=FORM + 1), W, T2, None, n), "common 129 is not -1"),
        "common 256": (lambda: ev(bent(common=256), W, T2, None, n), "common 256 is not -1"),
        "a summand's table at ntables": (lambda: ev(bent(table=2), W, T2, None, n), "form[0]: summand 0 names tables[2], ntables is 2"),
        "a summand's table a form": (lambda: ev(bent(table1=FORM), W, T2, None, n), "form[0]: summand 1 names tables[128]"),
        "a coefficient at ntables": (lambda: ev(bent(coef=2), W, T2, None, n), "form[0]: summand 0 takes its coefficient from tables[2], ntables is 2"),
        "a coefficient a form": (lambda: ev(bent(coef1=FORM), W, T2, None, n), "form[0]: summand 1 takes its coefficient from tables[128]"),
        "a bad form no term names": (lambda: ev(unused, W, T2, None, n), "form[1]: summand 0 names tables[2], ntables is 2"),
        "a bad second term": (lambda: ev(g(terms=[(1, [0]), (1, [1, 2])]), W, T2, None, n), "term[1]: factor 1 names tables[2]"),
        # negate and the reserved bytes
        "term negate 2": (lambda: ev(bent(term_negate=2), W, T2, None, n), "term[0]: negate 2 is neither 0 nor 1"),
        "summand negate 2": (lambda: ev(bent(negate=2), W, T2, None, n), "form[0]: summand 0: negate 2 is neither 0 nor 1"),
        "term reserved 0": (lambda: ev(bent(term_reserved=0), W, T2, None, n), "term[0]: a reserved byte is not 0"),
        "term reserved 1": (lambda: ev(bent(term_reserved=1), W, T2, None, n), "term[0]: a reserved byte is not 0"),
        "form reserved 0": (lambda: ev(bent(form_reserved=0), W, T2, None, n), "form[0]: a reserved byte is not 0"),
        "form reserved 2": (lambda: ev(bent(form_reserved=2), W, T2, None, n), "form[0]: a reserved byte is not 0"),
        "summand reserved": (lambda: ev(bent(reserved=1), W, T2, None, n), "form[0]: summand 0: the reserved byte is not 0"),
        # len
        "len 0": (lambda: ev(g(), W, T2, None, 0), "len 0: a gate evaluation with linear forms writes 1 <= len <= 256 words"),
        "len n + 1": (lambda: ev(g(), V(big.ptr, 0, 0, n), T2, None, n + 1), "len 257: a gate evaluation with linear forms writes 1 <= len <= 256 words"),
        "len above dst's count": (lambda: ev(g(), W8, [B0, B1], None, 9), "operand dst: count 8 is below the 9 words the op writes"),
        # the overlap rules
        "a table meeting dst off its start": (lambda: ev(g(), V(words.ptr + 32 * 4, 0, 0, 8), [B0, W], None, 8), "dst overlaps the words of tables[1] without starting where they start"),
        "a table inside dst": (lambda: ev(g(), W, [B0, V(words.ptr + 32 * 16, 0, 0, 1)], None, n), "dst overlaps the words of tables[1] without starting"),
        "a table at dst's start, rotated": (lambda: ev(g(), W, [W, B0], [1, 0], n), "dst names the words of tables[0], which is rotated by 1"),
        "a buffer at dst's start, rotated": (lambda: ev(g(), B1, [B0, B1], [0, n], n), "dst names the words of tables[1], which is rotated by 256"),
        "a table at dst's start, shorter than len": (lambda: ev(g(), W, [W8, B0], None, 9), "dst names the 8 words of tables[0], read periodically over len 9"),
        # operands, dst among them
        "tables[0] misaligned": (lambda: ev(g(), W, [V(words2.ptr + 8, 0, 0, 1), B0], None, n), "operand tables[0]: d_ptr is not 16-byte aligned"),
        "dst misaligned": (lambda: ev(g(), V(words.ptr + 8, 0, 0, 8), [B0, B1], None, 8), "operand dst: d_ptr is not 16-byte aligned"),
        "tables[1] in host memory": (lambda: ev(g(), W, [B0, V(host_ptr, 0, 0, n)], None, n), "operand tables[1]: d_ptr is not"),
        "dst in host memory": (lambda: ev(g(), V(host_ptr, 0, 0, n), [B0, B1], None, n), "operand dst: d_ptr is not"),
        "tables[0] reserved": (lambda: ev(g(), W, [V(None, 0, 7, 0), B1], None, n), "operand tables[0]: reserved must be 0"),
        "dst reserved": (lambda: ev(g(), V(words.ptr, 0, 1, n), [B0, B1], None, n), "operand dst: reserved must be 0"),
        "tables[1] buf 2": (lambda: ev(g(), W, [B0, V(None, 2, 0, 0)], None, n), "operand tables[1]: buf must be 0 or 1"),
        "dst buf 2": (lambda: ev(g(), V(None, 2, 0, 0), [B0, B1], None, n), "operand dst: buf must be 0 or 1"),
        "tables[1] buffer count": (lambda: ev(g(), W, [B0, V(None, 1, 0, 8)], None, n), "operand tables[1]: a transform buffer holds 256 elements, count says 8"),
        "tables[1] count 3": (lambda: ev(g(), W, [B0, V(words2.ptr, 0, 0, 3)], None, n), "operand tables[1]: count 3 is not a power of two"),
        "tables[0] count 2n": (lambda: ev(g(), W, [V(big.ptr, 0, 0, 2 * n), B1], None, n), "operand tables[0]: count 512 is not a power of two in [1, 256]"),
        "dst count 2n": (lambda: ev(g(), V(big.ptr, 0, 0, 2 * n), [B0, B1], None, n), "operand dst: count 512 is not a power of two in [1, 256]"),
        "tables[15] past its allocation": (lambda: ev(g(nt=16), W, [B0] * 15 + [V(words2.ptr + 32 * (n - 1), 0, 0, 2)], None, n), "operand tables[15]: 2 elements run past the end"),
        "dst past its allocation": (lambda: ev(g(), V(words.ptr + 32 * (n - 4), 0, 0, 8), [B0, B1], None, 8), "operand dst: 8 elements run past the end"),
    }
    out = _dev(fill(n, 9))
    for what, (attempt, message) in refused.items():
        assert attempt() == 4, what
        assert message in L.blz_last_error_message().decode(), (what, L.blz_last_error_message())
        with pytest.raises(DriverClientError) as ei:   # ... and nothing is in flight
            cl.wait_result()
        assert ei.value.variant == "InvalidPrimitiveParam", what
        assert bytes(words.download()) == bb, what   # dst is untouched
        assert ev(g(), out, [B0, B1], None, n) == 0, what   # and the handle still runs a good call
        cl.wait_result()
    assert bytes(out.download()) == _pack(lin_ref([a, b], FORMS, TERMS, None, r, n))
    with pytest.raises(DriverClientError) as ei:
        cl.gate_eval_lin(0, [0, 1], [], [(1, [0, 1, 0, 1, 0])])   # five factors: the library's to refuse
    assert ei.value.variant == "InvalidPrimitiveParam"
    with pytest.raises(DriverClientError) as ei:
        cl.gate_eval_lin(0, [0, 1], [[(1, None, 0)] * 5], [(1, [FORM])])   # five summands: likewise
    assert ei.value.variant == "InvalidPrimitiveParam"
    with pytest.raises(ValueError):
        cl.gate_eval_lin(0, [0, 1], FORMS, TERMS, rot=[1])
    with pytest.raises(ValueError):
        cl.gate_eval_lin(0, [0] * 17, FORMS, TERMS)
    # an op already in flight
    cl.vec_op(NTTClient.MUL, 1, 1, words2)
    assert ev(g(), W, [B0, W2], None, n) == 4 and "already running" in L.blz_last_error_message().decode()
    cl.reset()
    assert bytes(cl.result(0)) == ab
    assert bytes(words.download()) == bb and bytes(words2.download()) == ab and bytes(big.download()) == bytes(64 * n)
    cl.close()
    _free([words, words2, big, out])


def test_in_flight_rules(gpu):
    """With the op in flight the buffer written can be neither read, written nor exchanged, a buffer only read can be read but
    not written, and no transform, set_coset or op on the buffers starts.  wait_result finishes it, reset drops it."""
    field, logn = "BLS381", 8
    n = 1 << logn
    r = pyref.CURVES[field]["r"]
    a, b, c = (_inputs(r, n, 70 + i) for i in range(3))
    ab, bb, cb = _pack(a), _pack(b), _pack(c)
    cl = _client(field, logn)
    words, one_word, out = _dev(cb), _dev((7).to_bytes(32, "little")), DeviceBuffer(0, 32 * n)
    host_out = bytearray(32 * n)
    forms, terms = [[(1, None, 0), (-1, 1, 1)]], [(1, [FORM, 0])]   # (t0 - t1 t1) t0
    busy = (lambda: cl.start_process(0), lambda: cl.set_coset(7), lambda: cl.vec_op(NTTClient.MUL, 1, 1, words), lambda: cl.vec_reduce(NTTClient.FOLD_SUM, 0),
            lambda: cl.vec_mle_fold(1, 0, one_word), lambda: cl.sumcheck_gate([words], [(1, [0])]), lambda: cl.gate_eval(out, [words], [(1, [0])]),
            lambda: cl.gate_eval_lin(out, [words], [], [(1, [0])]), lambda: cl.gate_eval_lin(1, [0, words], forms, terms))
    cl.set_data(NTTInput(0, ab)); cl.set_data(NTTInput(1, bb))
    cl.gate_eval_lin(1, [0, words], forms, terms)   # writes buffer 1, reads buffer 0
    for attempt in busy + (lambda: cl.result(1), lambda: cl.set_data(NTTInput(1, ab)), lambda: cl.set_data(NTTInput(0, ab)),
                           lambda: cl.exchange(1, ab, host_out)):
        with pytest.raises(DriverClientError) as ei:
            attempt()
        assert ei.value.variant == "InvalidPrimitiveParam"
    assert bytes(cl.result(0)) == ab   # read-only: readable
    cl.wait_result()
    assert cl.last_kernel_ms() > 0
    want = lin_ref([a, c], forms, terms, None, r, n)
    assert bytes(cl.result(1)) == _pack(want) and bytes(cl.result(0)) == ab
    # dst in device words: both buffers are at most read
    f3, t3 = [[(1, 0, 1), (1, None, 2)]], [(1, [FORM])]
    cl.gate_eval_lin(out, [0, 1, words], f3, t3)
    assert bytes(cl.result(0)) == ab and bytes(cl.result(1)) == _pack(want)
    with pytest.raises(DriverClientError) as ei:
        cl.set_data(NTTInput(0, ab))
    assert ei.value.variant == "InvalidPrimitiveParam" and "buffer 0" in str(ei.value)
    for attempt in busy:
        with pytest.raises(DriverClientError):
            attempt()
    cl.wait_result()
    assert bytes(out.download()) == _pack(lin_ref([a, want, c], f3, t3, None, r, n))
    # reset with the op in flight: nothing is in flight afterwards, and the handle works
    cl.gate_eval_lin(1, [0, words], forms, terms)
    cl.reset()
    with pytest.raises(DriverClientError):
        cl.wait_result()
    cl.result(0); cl.result(1)
    cl.set_data(NTTInput(1, bb))
    f2 = [[(1, 0, 1), (1, None, 0)]]
    cl.gate_eval_lin(1, [0, 1], f2, [(1, [FORM, 1])])
    cl.wait_result()
    assert bytes(cl.result(1)) == _pack(lin_ref([a, b], f2, [(1, [FORM, 1])], None, r, n))
    cl.close()
    _free([words, one_word, out])
