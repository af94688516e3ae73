"""Cost of a verify pass against the float32 source (alac_hip_verify_float) and of the route a caller had before it:
    python tools/verify_float_timing.py [--out result.json] [--root CHECKOUT] [--packets 10000,125000] [--encode-only]
For 16- and 24-bit stereo, dither off and on, the source planar ([2, T] contiguous) and interleaved (the transposed view of
[T, 2]), every packet independent:
  verify_float      alac_hip_verify_float against the float source (skipped where the library has no such call)
  verify            alac_hip_verify against a prepared integer plane: the composed route's second half.  Its first half, the
                    quantize pass k_float_to_pcm, has no entry point of its own: take its time from a
                    `rocprofv3 --kernel-trace --stats -- python tools/verify_float_timing.py --encode-only` run (a run of its
                    own, no counters) and add it
  decode            alac_hip_decode, for scale
  decode_float, encode_float   the neighbouring float calls, for A/B runs of two builds
--root: import alac_amd from another checkout (one that holds its own built library), e.g. the parent commit's.
Times are device-synchronised wall times per call (best of 4 x 5 calls; inputs and outputs on the device)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--packets", default="10000,125000")
ap.add_argument("--encode-only", action="store_true", help="5 encode_float calls per shape and nothing else (profiler runs)")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))

import torch  # noqa: E402

import alac_amd  # noqa: E402

FS = 4096


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


def source(ctx, n, layout):
    """music-like float32 [2, n * FS] off the integer grid, planar or as the transposed view of [T, 2]"""
    g = torch.Generator(device="cuda").manual_seed(1)
    t = torch.arange(n * FS, device="cuda", dtype=torch.float32)
    x = torch.stack([0.4 * torch.sin(t * 0.01) + 0.2 * torch.sin(t * 0.0371), 0.4 * torch.sin(t * 0.011 + 1.0)])
    x = x + 1e-3 * torch.randn(x.shape, device="cuda", generator=g)
    return x.contiguous() if layout == "planar" else x.t().contiguous().t()


def measure(ctx, depth, n, dither, layout):
    fmt = alac_amd.make_format(FS, depth, 2, 44100)
    cookie = ctx.magic_cookie(fmt)
    key = dict(dither="tpdf", seed=7) if dither else {}
    r = {"depth": depth, "packets": n, "dither": dither, "layout": layout}
    with torch.cuda.stream(ctx.stream):
        x = source(ctx, n, layout)
        bufs = ctx.encode_buffers(fmt, n)
        b = ctx.encode_float(fmt, x, bufs=bufs, **key)
        ctx.synchronize()
        if ARGS.encode_only:
            for _ in range(5):
                ctx.encode_float(fmt, x, bufs=bufs, **key)
            ctx.synchronize()
            return r
        out = ctx.decode(cookie, b["out"], b["offsets"], n)  # the integer plane the stream decodes to = what was staged
        ctx.synchronize()
        plane = out[0].clone()
        fm, st, bad = ctx.verify(cookie, b["out"], b["offsets"], n, plane)
        ctx.synchronize()
        assert int(bad.item()) == 0, "verify reports a clean stream as bad"
        if hasattr(ctx, "verify_float"):
            fm, st, bad = ctx.verify_float(cookie, b["out"], b["offsets"], n, x, **key)
            ctx.synchronize()
            assert int(bad.item()) == 0 and bool((fm == -1).all()), "verify_float reports a clean stream as bad"
            r["verify_float_ms"] = best_of(ctx, lambda: ctx.verify_float(cookie, b["out"], b["offsets"], n, x, **key)) * 1e3
        r["verify_ms"] = best_of(ctx, lambda: ctx.verify(cookie, b["out"], b["offsets"], n, plane)) * 1e3
        r["decode_ms"] = best_of(ctx, lambda: ctx.decode(cookie, b["out"], b["offsets"], n, out=out[:3])) * 1e3
        fo = ctx.decode_float(cookie, b["out"], b["offsets"], n)
        ctx.synchronize()
        r["decode_float_ms"] = best_of(ctx, lambda: ctx.decode_float(cookie, b["out"], b["offsets"], n, out=fo[:3])) * 1e3
        r["encode_float_ms"] = best_of(ctx, lambda: ctx.encode_float(fmt, x, bufs=bufs, **key)) * 1e3
    print(json.dumps(r), flush=True)
    return r


def main():
    ctx = alac_amd.Context(0)
    res = []
    for n in [int(v) for v in ARGS.packets.split(",")]:
        for depth in (16, 24):
            for dither in (False, True):
                for layout in ("planar", "interleaved"):
                    res.append(measure(ctx, depth, n, dither, layout))
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump({"library": alac_amd.LIB_PATH, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
