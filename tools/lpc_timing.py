"""Codec time of the LPC encode mode (option "lpc") against the modes it sits between:  python tools/lpc_timing.py
  * one 50.wav-sized file (the reference's audio/50.wav, 237 stereo packets, from tests/golden): chained (one segment),
    K = 1 (every packet its own segment) and lpc, with the stream size of each
  * BASELINE configs[1]: 10 000 synthetic 16-bit stereo packets, every packet independent, with and without lpc, and the
    decode time of both streams (LPC channels of order > 8 or denShift != 9 take the decoder's generic predictor)
Times are device-synchronised wall times of the encode call (best of 4 x 5 calls, inputs and outputs on the device)."""
import json
import lzma
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import alac_amd  # noqa: E402


def timed(ctx, fmt, d_pcm, n, label, **kw):
    with torch.cuda.stream(ctx.stream):
        b = ctx.encode(fmt, d_pcm, n, **kw)
        ctx.synchronize()
        best = 1e9
        for _ in range(4):
            t = time.perf_counter()
            for _ in range(5):
                ctx.encode(fmt, d_pcm, n, bufs=b, **kw)
            ctx.synchronize()
            best = min(best, (time.perf_counter() - t) / 5)
    print(f"{label}: {best * 1e3:.3f} ms, {int(b['offsets'][-1].item())} B", flush=True)
    return best, b


def timed_decode(ctx, fmt, b, n, want, label):
    cookie = ctx.magic_cookie(fmt)
    with torch.cuda.stream(ctx.stream):
        out = ctx.decode(cookie, b["out"], b["offsets"], n)
        ctx.synchronize()
        assert torch.equal(out[0], want), "round trip differs"
        best = 1e9
        for _ in range(4):
            t = time.perf_counter()
            for _ in range(5):
                ctx.decode(cookie, b["out"], b["offsets"], n, out=out[:3])
            ctx.synchronize()
            best = min(best, (time.perf_counter() - t) / 5)
    print(f"{label}: {best * 1e3:.3f} ms", flush=True)
    return best


def main():
    ctx = alac_amd.Context(0)
    with open(os.path.join(ROOT, "tests", "golden", "wav50_pcm.xz"), "rb") as f:
        pcm = np.frombuffer(lzma.decompress(f.read()), np.uint8)
    fmt = alac_amd.make_format(4096, 16, 2, 44100)
    n = (pcm.size // fmt.bytes_per_frame + 4095) // 4096
    padded = np.zeros(n * fmt.packet_bytes, np.uint8)
    padded[:pcm.size] = pcm
    d_pcm = torch.from_numpy(padded).cuda()
    ns = np.full(n, 4096, np.uint32)
    ns[-1] = pcm.size // fmt.bytes_per_frame - (n - 1) * 4096
    d_ns = torch.from_numpy(ns.view(np.int32)).cuda()
    seg = torch.tensor([0, n], dtype=torch.int32).cuda()
    out = {}
    out["file_chained_ms"] = timed(ctx, fmt, d_pcm, n, f"50.wav ({n} packets) chained", num_samples=d_ns, seg_first=seg,
                                   max_segment_packets=n)[0] * 1e3
    out["file_k1_ms"] = timed(ctx, fmt, d_pcm, n, f"50.wav ({n} packets) K = 1", num_samples=d_ns)[0] * 1e3
    with ctx.options(lpc=1):
        out["file_lpc_ms"] = timed(ctx, fmt, d_pcm, n, f"50.wav ({n} packets) lpc", num_samples=d_ns)[0] * 1e3
    n = 10000
    d_pcm = ctx.synth_pcm(0, n, fmt)
    t, b = timed(ctx, fmt, d_pcm, n, f"configs[1] {n} packets")
    out["batch_default_ms"] = t * 1e3
    out["decode_default_ms"] = timed_decode(ctx, fmt, b, n, d_pcm, "decode of that stream") * 1e3
    with ctx.options(lpc=1):
        t, b = timed(ctx, fmt, d_pcm, n, f"configs[1] {n} packets lpc")
    out["batch_lpc_ms"] = t * 1e3
    out["decode_lpc_ms"] = timed_decode(ctx, fmt, b, n, d_pcm, "decode of the lpc stream") * 1e3
    print(json.dumps({k: round(v, 3) for k, v in out.items()}))


if __name__ == "__main__":
    main()
