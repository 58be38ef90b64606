"""What the device tests of the ops on resident buffers share (test_gpu_ntt_vec.py, test_gpu_ntt_fold.py,
test_gpu_ntt_horner.py): the wire format, the input recipe's pieces - the edge words 0, 1, r - 1, r, r + 1, 2^256 - 1 and
unmasked random 256-bit words - and the handle's plumbing.  Each file keeps its own _inputs and seeds."""
import random

from blaze_amd import DeviceBuffer
from blaze_amd.driver_client import DriverClient
from blaze_amd.ingo_ntt import NTT, NTTClient, NttInit

FIELDS = ["BLS381", "BLS377", "BN254"]
GENERATOR = {"BLS381": 7, "BLS377": 22, "BN254": 5}   # the fields' multiplicative generators
TOP = (1 << 256) - 1


def _pack(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def _unpack(data):
    data = bytes(data)
    return [int.from_bytes(data[i: i + 32], "little") for i in range(0, len(data), 32)]


def _words(seed, count):
    """Random 256-bit words, no top-byte mask: more than half of them are >= r in every field."""
    raw = random.Random(seed).randbytes(32 * count)
    return [int.from_bytes(raw[i: i + 32], "little") for i in range(0, len(raw), 32)]


def _edges(r):
    return [0, 1, r - 1, r, r + 1, TOP]


def _client(field, logn, **kw):
    return NTTClient(NTT.Ntt, DriverClient(0), log_size=logn, field=field, **kw)


def _dev(data):
    d = DeviceBuffer(0, len(data))
    d.upload(data)
    return d


def _word(d):
    return int.from_bytes(bytes(d.download(32)), "little")


def _transform(cl, buf):
    cl.initialize(NttInit())
    cl.start_process(buf)
    cl.wait_result()
