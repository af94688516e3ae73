"""Cost of a verify pass (alac_hip_verify) against a decode pass:  python tools/verify_timing.py [--out result.json]
For 10 000 and 125 000 synthetic 16-bit stereo packets (BASELINE configs[1] / the configs[3] shard), every packet independent:
  decode            alac_hip_decode into a device buffer
  verify            alac_hip_verify against the source PCM on the device, one word (the bad-packet count) read back
  decode+d2h+host   what a caller did before: decode, copy the whole PCM to the host, compare there with numpy
Times are device-synchronised wall times per call (best of 4 x 5 calls; inputs and outputs on the device); the host compare
is timed on its own and added."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import alac_amd  # noqa: E402


def best_of(ctx, fn, reps=5, rounds=4):
    ctx.synchronize()
    best = 1e9
    for _ in range(rounds):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.synchronize()
        best = min(best, (time.perf_counter() - t) / reps)
    return best


def measure(ctx, n):
    fmt = alac_amd.make_format(4096, 16, 2, 44100)
    d_pcm = ctx.synth_pcm(0, n, fmt)
    cookie = ctx.magic_cookie(fmt)
    r = {"packets": n}
    with torch.cuda.stream(ctx.stream):
        b = ctx.encode(fmt, d_pcm, n)
        ctx.synchronize()
        out = ctx.decode(cookie, b["out"], b["offsets"], n)
        ctx.synchronize()
        assert torch.equal(out[0], d_pcm), "round trip differs"
        fm, st, bad = ctx.verify(cookie, b["out"], b["offsets"], n, d_pcm)
        ctx.synchronize()
        assert int(bad.item()) == 0 and bool((fm == -1).all()), "verify reports a clean stream as bad"
        r["decode_ms"] = best_of(ctx, lambda: ctx.decode(cookie, b["out"], b["offsets"], n, out=out[:3])) * 1e3
        r["verify_ms"] = best_of(ctx, lambda: ctx.verify(cookie, b["out"], b["offsets"], n, d_pcm)) * 1e3
        host_pcm = d_pcm.cpu().numpy()
        pinned = torch.empty(out[0].numel(), dtype=torch.uint8, pin_memory=True)

        def d2h():
            ctx.decode(cookie, b["out"], b["offsets"], n, out=out[:3])
            pinned.copy_(out[0], non_blocking=True)

        r["decode_d2h_ms"] = best_of(ctx, d2h) * 1e3
        got = pinned.numpy()
        t = time.perf_counter()
        for _ in range(3):
            assert np.array_equal(got, host_pcm)
        r["host_compare_ms"] = (time.perf_counter() - t) / 3 * 1e3
    r["decode_d2h_host_ms"] = r["decode_d2h_ms"] + r["host_compare_ms"]
    r["verify_over_decode"] = r["verify_ms"] / r["decode_ms"]
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--packets", default="10000,125000")
    a = ap.parse_args()
    ctx = alac_amd.Context(0)
    res = [measure(ctx, int(x)) for x in a.packets.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
