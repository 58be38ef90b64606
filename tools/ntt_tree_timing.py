#!/usr/bin/env python3
"""What the product and fraction trees cost over the BLS12-381 scalar field (blz_ntt_mle_tree; DESIGN.md section 4, "Product and
fraction trees"): medians of blz_ntt_last_kernel_ms and of the wall time with min - max, every leg alternating in the same process
with its two yardsticks - the shortest sequence of existing ops that writes the same bytes, one layer at a time over views of the
same memory, each op with its blz_ntt_wait_result (kernel times summed; the sequence is written into the JSON), and a
device-to-device hipMemcpyAsync of half the bytes the fused op moves, which moves as many.
    prod        the product tree, top-variable pairing: per layer one gate_eval(lo hi) over the two halves of the layer below
    frac        the fraction tree: per layer gate_eval(P_lo Q_hi + P_hi Q_lo) and gate_eval(Q_lo Q_hi)
    prod_low    the product tree pairing (2p, 2p + 1): per layer two vec_gather (stride 2) into the transform buffers and one
                gate_eval over them
at len = 2^24 and, where memory allows, 2^27.  The outputs are checked on the device before anything is written: a DOT of every
destination with a random vector after the fused op equals the one after the sequence.  Writes profiles/ntt_tree_ops.json.  The
device work runs in ONE child process under its own time limit.

    python tools/ntt_tree_timing.py [--out profiles/ntt_tree_ops.json] [--rounds 9] [--timeout 900] [--no-large]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOP_WORDS = 1024            # csrc/ntt_tree.hip.hpp TREE_TOP: one block finishes from here
LEVELS = {"prod": 3, "frac": 2, "prod_low": 3}   # tree_levels(): layers a launch of k_tree_up keeps in registers
PRODUCTS = {"prod": 2, "frac": 5, "prod_low": 2}  # Montgomery products per node, fused; the sequence's gate_eval: 2 and 4 + 2


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]}


def words_moved(length, levels, tables):
    """the words the fused op reads and writes: the leaves, every layer, and the top layer of every launch but the last again"""
    again, cur = 0, length
    while cur > TOP_WORDS:
        cur >>= levels
        again += cur
    return tables * (length + length - 1 + again)


def child(rounds: int, large: bool) -> dict:
    import blaze_amd
    from blaze_amd import DeviceBuffer
    from blaze_amd._lib import check, lib
    from blaze_amd.driver_client import DriverClient
    from blaze_amd.ingo_ntt import NTT, NTTClient

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]

    def hip_ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with hipError {rc}")

    DOT, PROD, FRAC = NTTClient.FOLD_DOT, NTTClient.TREE_PROD, NTTClient.TREE_FRAC
    dc = DriverClient(0)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    hip_ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    def size_case(logn):
        n = 1 << logn
        cl = NTTClient(NTT.Ntt, dc, log_size=logn, flags=NTTClient.NO_FACTOR_TABLE)
        stream, dev = C.c_void_p(), C.c_int()
        check(lib().blz_ntt_stream(cl._h, C.byref(stream), C.byref(dev)))
        src = [DeviceBuffer(0, 32 * n) for _ in range(2)]     # P, Q
        tree = [DeviceBuffer(0, 32 * n) for _ in range(2)]    # the fused op's destinations
        seq = [DeviceBuffer(0, 32 * n) for _ in range(2)]     # the sequence's
        w = DeviceBuffer(0, 32 * n)
        for i, d in enumerate(src + [w]):
            check(blaze_amd.aux().blz_synth_field_elements(0, d.ptr, n, 431 + i))
        for d in tree + seq:   # word n - 1 is nobody's: the same bytes in both
            hip_ok(hip.hipMemsetAsync(d.ptr, 0, 32 * n, stream), "hipMemsetAsync")
        hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

        def layer(buf, k):
            """(lo half, hi half, whole) of layer k of a destination; k == 0: of the source"""
            off, words = (0, n) if k == 0 else NTTClient.tree_layer(n, k)
            whole = buf.view(32 * off, 32 * words)
            if words == 1:
                return whole, whole, whole
            return buf.view(32 * off, 16 * words), buf.view(32 * off + 16 * words, 16 * words), whole

        def op(f, *args, **kw):
            f(*args, **kw)
            cl.wait_result()
            return cl.last_kernel_ms()

        def timed(f):
            t0 = time.perf_counter()
            ms = f()
            return ms, (time.perf_counter() - t0) * 1e3

        def digest(d):
            x = cl.vec_reduce(DOT, d, w)
            cl.wait_result()
            got = bytes(x.download())
            x.free()
            return got

        def prod_sequence():
            ms = []
            for k in range(1, logn + 1):
                lo, hi, _ = layer(src[0] if k == 1 else seq[0], k - 1)
                ms.append(op(cl.gate_eval, layer(seq[0], k)[2], [lo, hi], [(1, [0, 1])], length=n >> k))
            return sum(ms)

        def frac_sequence():
            ms = []
            for k in range(1, logn + 1):
                plo, phi, _ = layer(src[0] if k == 1 else seq[0], k - 1)
                qlo, qhi, _ = layer(src[1] if k == 1 else seq[1], k - 1)
                ms.append(op(cl.gate_eval, layer(seq[0], k)[2], [plo, phi, qlo, qhi], [(1, [0, 3]), (1, [1, 2])], length=n >> k))
                ms.append(op(cl.gate_eval, layer(seq[1], k)[2], [qlo, qhi], [(1, [0, 1])], length=n >> k))
            return sum(ms)

        def prod_low_sequence():
            ms = []
            for k in range(1, logn + 1):
                below = layer(src[0] if k == 1 else seq[0], k - 1)[2]
                ms.append(op(cl.vec_gather, 0, below, offset=0, stride=2, length=n >> k))
                ms.append(op(cl.vec_gather, 1, below, offset=1, stride=2, length=n >> k))
                ms.append(op(cl.gate_eval, layer(seq[0], k)[2], [0, 1], [(1, [0, 1])], length=n >> k))
            return sum(ms)

        def leg(name, fused, sequence, names, tables):
            moved = 32 * words_moved(n, LEVELS[name], tables)
            half = (moved // 2 + 255) & ~255
            c_src, c_dst = DeviceBuffer(0, half), DeviceBuffer(0, half)
            hip_ok(hip.hipMemsetAsync(c_src.ptr, 1, half, stream), "hipMemsetAsync")
            hip_ok(hip.hipMemsetAsync(c_dst.ptr, 2, half, stream), "hipMemsetAsync")
            hip_ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")

            def copy():
                ms = C.c_float()
                hip_ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
                hip_ok(hip.hipMemcpyAsync(c_dst.ptr, c_src.ptr, half, 3, stream), "hipMemcpyAsync")   # hipMemcpyDeviceToDevice
                hip_ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
                hip_ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
                hip_ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
                return float(ms.value)

            # the outputs first: the same bytes, and not all zero
            fused()
            sequence()
            for t in range(tables):
                want = digest(seq[t])
                if digest(tree[t]) != want or not any(want):
                    raise RuntimeError(f"2^{logn} {name}: destination {t} of the fused op differs from the sequence's")
            f_ms, f_wall, s_ms, s_wall, c_ms = [], [], [], [], []
            for it in range(rounds + 2):   # two warm-up rounds
                (x, xw), (y, yw), z = timed(fused), timed(sequence), copy()
                if it >= 2:
                    f_ms.append(x); f_wall.append(xw); s_ms.append(y); s_wall.append(yw); c_ms.append(z)
            for d in (c_src, c_dst):
                d.free()
            fs, ss, cs = stats(f_ms), stats(s_ms), stats(c_ms)
            fw, sw = stats(f_wall), stats(s_wall)
            # per node of a layer the sequence moves: prod 2 read + 1 written; frac (4 + 1) + (2 + 1); prod_low two gathers (1 read
            # each, and the whole buffer written: zero fill) and 2 + 1
            seq_words = {"prod": 3 * (n - 1), "frac": 8 * (n - 1), "prod_low": 5 * (n - 1) + 2 * n * logn}[name]
            return {"len": n, "products_per_node": PRODUCTS[name], "launches": -(-max(logn - 10, 0) // LEVELS[name]) + 1,
                    "bytes_moved": moved, "sequence_bytes_moved": 32 * seq_words, "traffic_predicts_fused_to_sequence": round(moved / (32 * seq_words), 4),
                    "mle_tree": fs, "mle_tree_wall": fw, "sequence_of_existing_ops": names, "sequence_ops": len(names) * logn, "sequence": ss, "sequence_wall": sw,
                    "copy_of_the_bytes_moved": cs,
                    "fused_to_sequence": round(fs["median_ms"] / ss["median_ms"], 4), "fused_to_sequence_wall": round(fw["median_ms"] / sw["median_ms"], 4),
                    "fused_to_copy": round(fs["median_ms"] / cs["median_ms"], 4),
                    "fused_range_below_sequence_range": fs["min_max_ms"][1] < ss["min_max_ms"][0],
                    "achieved_tb_per_s": round(moved / fs["median_ms"] / 1e9, 3), "checked": True}

        res = {
            "prod": leg("prod", lambda: op(cl.mle_tree, tree[0], src[0]), prod_sequence, ["layer k = gate_eval(lo hi) over the halves of layer k - 1"], 1),
            "frac": leg("frac", lambda: op(cl.mle_tree, tree[0], src[0], FRAC, dst_q=tree[1], a_q=src[1]), frac_sequence,
                        ["P layer k = gate_eval(P_lo Q_hi + P_hi Q_lo)", "Q layer k = gate_eval(Q_lo Q_hi)"], 2),
            "prod_low": leg("prod_low", lambda: op(cl.mle_tree, tree[0], src[0], low=True), prod_low_sequence,
                            ["buf0 = vec_gather(layer k - 1, offset 0, stride 2)", "buf1 = vec_gather(layer k - 1, offset 1, stride 2)", "layer k = gate_eval(buf0 buf1)"], 1),
        }
        for d in src + tree + seq + [w]:
            d.free()
        cl.close()
        return res

    res = {"field": "BLS381", "rounds": rounds, "2^24": size_case(24)}
    if large:
        try:
            res["2^27"] = size_case(27)
        except blaze_amd.DriverClientError as e:   # the memory for it (some 45 GiB) is not there: the smaller size stands alone
            res["2^27"] = {"skipped": str(e)[:200]}
    cal = (C.c_double * 4)()
    check(blaze_amd.aux().blz_calib_mad_rate(0, 50, cal))
    res["calib_mad_rate"], res["calib_clock_mhz"] = cal[0], cal[2]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt_tree_ops.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--no-large", action="store_true", help="leave the 2^27 case out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.rounds, not a.no_large)))
        return 0
    r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds)]
                       + (["--no-large"] if a.no_large else []), capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f"the measuring process ended with status {r.returncode}: nothing written")
        return r.returncode
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
