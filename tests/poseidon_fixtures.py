"""Poseidon instruction CSVs for the tests.  The files are 40 - 130 KB of decimal text each, so they are not committed: they are
written by tools/poseidon_params.py on first use into a per-user cache directory, and tests/golden/poseidon_params.json pins every
byte of them by SHA-256 (the tool is deterministic; a change of its output is a change of the digest)."""
import hashlib
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PINNED = json.load(open(os.path.join(HERE, "golden", "poseidon_params.json")))


def tool():
    """tools/poseidon_params.py as a module"""
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import poseidon_params
    return poseidon_params


def generate(name) -> bytes:
    """the tool's CSV for the pinned configuration `name`, as it would write it"""
    spec = PINNED[name]
    return tool().csv_text(tool().generate(spec["field"], [tuple(b) for b in spec["blocks"]])).encode()


def with_random_matrices(words, r, seed):
    """a copy of the word stream with every block's t^2 MDS words replaced by random field elements: NOT symmetric (the tool's Cauchy
    matrices 1 / (i + t + j) are), so it tells a row-major matrix product from its transpose.  The loader accepts any words < r."""
    w, pos, rng = list(words), 3, random.Random(seed)
    for _ in range(w[2]):
        t, _alpha, rf, rp = w[pos:pos + 4]
        m = pos + 5 + t * (rf + rp)
        for k in range(t * t):
            w[m + k] = rng.randrange(r)
        pos = m + t * t
    return w


def path(name) -> str:
    """path of the CSV for `name` ("bls381_t9_t12": t = 9 and 12 with (8, 57) rounds; "<field>_small": t = 3, 9, 12 with (8, 5))"""
    want = PINNED[name]["sha256"]
    d = os.path.join(tempfile.gettempdir(), f"blaze_poseidon_params_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    p = os.path.join(d, f"poseidon_{name}.csv")
    if not (os.path.exists(p) and hashlib.sha256(open(p, "rb").read()).hexdigest() == want):
        text = generate(name)
        assert hashlib.sha256(text).hexdigest() == want, f"tools/poseidon_params.py no longer writes the pinned bytes of {name}"
        tmp = f"{p}.{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(text)
        os.replace(tmp, p)
    return p
