"""The optimised partial rounds in Python integers: the derivation of include/blaze_hip.h "ROUNDS" / DESIGN.md section 8 and the
permutation that runs on the derived tables.  A model of what the device derives (k_hades_derive) and runs (k_hades_hash), to be
compared with the dense definition, poseidon_ref.permute.

Round = add constants -> S-box -> state <- M state.  M = [[m00, v^T], [w, Mh]], Mh the lower-right (t-1) x (t-1) block, P = R_P.
For the partial rounds k = 1 .. P put j = P - k + 1 and substitute state = diag(1, Mh^-(j-1)) z behind round k: diag(1, A) commutes
with the partial S-box, so round k becomes  z <- S_k sbox0(z + c'_k)  with
    S_k  = [[m00, v^T Mh^-j], [Mh^(j-1) w, I]]      (2t - 1 entries that are not 0 or 1)
    c'_k = diag(1, Mh^j) c_k
and the full round in front of them multiplies by diag(1, Mh^P) M.  Behind round P the substitution is the identity."""


class Singular(Exception):
    """Mh has no inverse: the width does not admit the optimised rounds"""


def mat_mul(a, b, r):
    return [[sum(x * y for x, y in zip(row, col)) % r for col in zip(*b)] for row in a]


def mat_vec(a, x, r):
    return [sum(m * y for m, y in zip(row, x)) % r for row in a]


def vec_mat(x, a, r):
    return [sum(y * row[c] for y, row in zip(x, a)) % r for c in range(len(a[0]))]


def identity(n):
    return [[int(i == j) for j in range(n)] for i in range(n)]


def invert(a, r):
    """Gauss-Jordan, a Fermat inverse per pivot; Singular when a column has no pivot"""
    n = len(a)
    a = [list(row) + ident for row, ident in zip(a, identity(n))]
    for c in range(n):
        p = next((i for i in range(c, n) if a[i][c] % r), None)
        if p is None:
            raise Singular(f"no pivot in column {c}")
        a[c], a[p] = a[p], a[c]
        inv = pow(a[c][c], r - 2, r)
        a[c] = [x * inv % r for x in a[c]]
        for i in range(n):
            if i != c and a[i][c]:
                f = a[i][c]
                a[i] = [(x - f * y) % r for x, y in zip(a[i], a[c])]
    return [row[n:] for row in a]


def derive(blk, r):
    """dict(sparse = [(u_k, w_k)] for k = 1 .. P with u_k[0] = m00 and w_k[0] unused (0), rc = the P transformed constant rows,
    pre = the matrix of the last full round of the first half); raises Singular"""
    t, rf, rp = blk["t"], blk["rf"], blk["rp"]
    m = [[x % r for x in row] for row in blk["mds"]]
    if rp == 0:
        return dict(sparse=[], rc=[], pre=m)
    mh = [row[1:] for row in m[1:]]
    v, w = m[0][1:], [row[0] for row in m[1:]]
    mh_inv = invert(mh, r)
    sparse, rc = [None] * rp, [None] * rp
    u, wk, pw = list(v), list(w), identity(t - 1)       # v^T Mh^-(j-1), Mh^(j-1) w, Mh^(j-1)
    for j in range(1, rp + 1):
        k = rp - j + 1
        u = vec_mat(u, mh_inv, r)
        pw = mat_mul(pw, mh, r)
        c = blk["rc"][rf // 2 + k - 1]
        sparse[k - 1] = ([m[0][0]] + u, [0] + wk)
        rc[k - 1] = [c[0] % r] + mat_vec(pw, c[1:], r)
        wk = mat_vec(mh, wk, r)
    pre = [m[0]] + mat_mul(pw, m[1:], r)                # diag(1, Mh^P) M
    return dict(sparse=sparse, rc=rc, pre=pre)


def permute(state, blk, r, tables=None):
    """the permutation on the derived tables: R_F / 2 dense full rounds (the last one with `pre`), P sparse rounds, R_F / 2 dense"""
    t, rf, rp = blk["t"], blk["rf"], blk["rp"]
    d = tables or derive(blk, r)
    half = rf // 2
    s = [x % r for x in state]
    assert len(s) == t
    for rnd in range(half):
        s = [pow((x + c) % r, 5, r) for x, c in zip(s, blk["rc"][rnd])]
        s = mat_vec(d["pre"] if rnd == half - 1 else blk["mds"], s, r)
    for (u, w), c in zip(d["sparse"], d["rc"]):
        y = [(x + cc) % r for x, cc in zip(s, c)]
        y[0] = pow(y[0], 5, r)
        s = [sum(a * b for a, b in zip(u, y)) % r] + [(w[i] * y[0] + y[i]) % r for i in range(1, t)]
    for rnd in range(half + rp, rf + rp):
        s = [pow((x + c) % r, 5, r) for x, c in zip(s, blk["rc"][rnd])]
        s = mat_vec(blk["mds"], s, r)
    return s


def hash_fixed(inputs, blk, r, tables=None):
    assert len(inputs) == blk["t"] - 1
    return permute([blk["tag"]] + list(inputs), blk, r, tables)[1]
