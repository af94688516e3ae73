"""Whole-call times of the encode family, for comparing two builds of the library in alternating processes:
    ALAC_HIP_LIB=/path/to/libalac_hip.so python tools/encode_call_timing.py --out result.json
    python tools/encode_call_timing.py --table parent1.json branch1.json parent2.json branch2.json ...
One process measures `encode`, `encode_float`, `encode_int` (planar int32, left-justified) and `encode_host_segments` on 16-bit
stereo at 24 and at 10 000 packets of 4096 frames, every packet its own segment, and `encode` with 6 channels at 24 packets;
each twice (pass 1, pass 2), so that a drift inside a process shows.  A device form is timed between two events on the
context's stream around one call, inputs, workspace and outputs on the device and allocated once (rounds_ms of
tools/decode_int_timing.py: the median of 7 rounds of the median of 10 calls, 3 warm-up calls in front); the host form, which
returns when its results are in host memory, by the host's clock around the call, in the same rounds.
--table prints the rows of profiles/encode_call/ab.md from the results of alternating processes (parent first in every pair)
with the bar of profiles/decode_call/ab.md: the branch's median of its per-process medians inside the parent's [smallest,
largest] per-process median, widened on both sides by the branch's own spread."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FRAME = 4096
CALLS = [("encode", 2, 24), ("encode_float", 2, 24), ("encode_int", 2, 24), ("encode_host_segments", 2, 24),
         ("encode", 6, 24), ("encode", 2, 10000), ("encode_float", 2, 10000), ("encode_int", 2, 10000),
         ("encode_host_segments", 2, 10000)]


def host_rounds_ms(fn, reps=10, warm=3, rounds=7):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(rounds):
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e3)
        out.append(statistics.median(times))
    return {"ms": statistics.median(out), "spread_ms": [min(out), max(out)]}


def measure(out_path):
    import numpy as np
    import torch
    import alac_amd
    from decode_int_timing import rounds_ms
    ctx = alac_amd.Context(0)
    lib = ctx.lib
    rows = []
    for pas in (1, 2):
        for call, channels, n in CALLS:
            fmt = alac_amd.make_format(FRAME, 16, channels, 44100)
            pcm = alac_amd.synth_pcm(0, n, fmt)
            val = np.ascontiguousarray(pcm.view(np.int16).reshape(-1, channels).T)  # [C, T]
            bufs = ctx.encode_buffers(fmt, n)
            if call == "encode":
                d = torch.from_numpy(pcm).cuda()
                r = rounds_ms(ctx, lambda: ctx.encode(fmt, d, n, bufs=bufs))
            elif call == "encode_float":
                d = torch.from_numpy((val / 32768.0).astype(np.float32)).cuda()
                r = rounds_ms(ctx, lambda: ctx.encode_float(fmt, d, bufs=bufs))
            elif call == "encode_int":
                d = torch.from_numpy(val.astype(np.int32) << 16).cuda()
                r = rounds_ms(ctx, lambda: ctx.encode_int(fmt, d, bufs=bufs))
            else:
                ns = np.full(n, FRAME, np.uint32)
                seg = np.arange(n + 1, dtype=np.uint32)
                cap = int(lib.alac_hip_encode_max_output_bytes(C.byref(fmt), n))
                out, sizes, total = np.empty(cap, np.uint8), np.empty(n, np.uint32), C.c_uint64(0)

                def host():
                    rc = lib.alac_hip_encode_host_segments(ctx.h, C.byref(fmt), pcm.ctypes.data, ns.ctypes.data, n, seg.ctypes.data, n,
                                                           None, 0, out.ctypes.data, cap, sizes.ctypes.data, C.byref(total))
                    assert rc == 0, rc
                r = host_rounds_ms(host)
            rows.append({"call": call, "channels": channels, "packets": n, "pass": pas, **r})
            print(rows[-1], flush=True)
    with open(out_path, "w") as f:
        json.dump({"library": alac_amd.capi.LIB_PATH, "rows": rows}, f, indent=1)


def table(paths):
    runs = [json.load(open(p))["rows"] for p in paths]
    parent, branch = runs[0::2], runs[1::2]
    print("| call | channels | packets | pass | parent: median per process (ms) | branch: median per process (ms) | branch's own spread "
          "(ms) | window (ms) | branch median (ms) | branch / parent | verdict |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for i, row in enumerate(parent[0]):
        p, b = [r[i]["ms"] for r in parent], [r[i]["ms"] for r in branch]
        spread, med = max(b) - min(b), statistics.median(b)
        lo, hi = min(p) - spread, max(p) + spread
        verdict = "inside" if lo <= med <= hi else ("SLOWER" if med > hi else "faster")
        f = lambda xs: " ".join("%.4f" % x for x in xs)
        print("| `%s` | %d | %d | %d | %s | %s | %.4f | %.4f .. %.4f | %.4f | %.4f | %s |" % (
            row["call"], row["channels"], row["packets"], row["pass"], f(p), f(b), spread, lo, hi, med,
            med / statistics.median(p), verdict))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="encode_call_timing.json")
    ap.add_argument("--table", nargs="+")
    a = ap.parse_args()
    table(a.table) if a.table else measure(a.out)
