"""Cost of converting the sample rate where the PCM lies (alac_hip_resample_int) against the true-peak call on the same plane
(alac_hip_true_peak_int, the same arithmetic with the outputs reduced to a maximum) and against reading the source once
(alac_hip_int_probe).
    python tools/resample_timing.py [--out result.json] [--packets 10000,125000]
For 10 000 and 125 000 packets of 4096 16-bit stereo frames (the synthetic PCM, interleaved, in the layout alac_hip_decode
writes), at 44.1 -> 48 kHz and at 96 -> 44.1 kHz, in one process:
  resample_1024     alac_hip_resample_int with a table of 1 024 equal segments
  resample_1        the same call with one segment
  true_peak_1024    alac_hip_true_peak_int on the same plane and table (as 44.1 kHz material: the 4x interpolator)
  probe_1024        alac_hip_int_probe on the same source and table: the cost of reading it once
  host_scipy_s      where scipy is present, at 10 000 packets: the copy to the host plus scipy.signal.resample_poly, seconds
The bar, per shape: per input frame and channel the call does K L / M fused multiply-adds (87 at 160/147, 81 at 147/320), the
true-peak call 36 * 64 / 53 = 43.5, so
  bar               resample_1024 <= true_peak_1024 * (K L / M) / 43.5, widened by both spreads (max - min of the 7 rounds;
                    the true-peak call's scaled as its median is)
The outputs of the first 16 packets are compared with the restatement (tests/resample_ref.py) before anything is timed.
GPU times are milliseconds between two events on the context's stream around 10 calls, divided by 10: the median of 7 such
rounds after one warm-up round, with [min, max]."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import alac_amd  # noqa: E402
import resample_ref as rr  # noqa: E402

PAIRS = [(44100, 48000), (96000, 44100)]
TRUE_PEAK_FMA = 36.0 * 64.0 / 53.0


def rounds_ms(ctx, fn, rounds=7, calls=10):
    times = []
    for r in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ctx.stream)
        for _ in range(calls):
            fn()
        b.record(ctx.stream)
        b.synchronize()
        if r:
            times.append(a.elapsed_time(b) / calls)
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def bar(got, limit, factor):
    """got <= factor * limit, widened by the two spreads"""
    slack = (got["max"] - got["min"]) + factor * (limit["max"] - limit["min"])
    return {"met": got["median"] <= factor * limit["median"] + slack, "got_ms": got["median"],
            "limit_ms": factor * limit["median"], "factor": factor, "slack_ms": slack}


def measure(ctx, n, rates, with_scipy):
    fmt = alac_amd.make_format(4096, 16, 2, rates[0])
    frames = n * 4096
    L, M, coefs = alac_amd.resample_filter(*rates)
    K = coefs.shape[1]
    r = {"packets": n, "frames": frames, "in_rate": rates[0], "out_rate": rates[1], "L": L, "M": M, "K": K,
         "fma_per_input_sample": K * L / M, "pcm_bytes": n * fmt.packet_bytes}
    with torch.cuda.stream(ctx.stream):
        pcm = ctx.synth_pcm(0, n, fmt)
        x = pcm.view(torch.int16).view(frames, 2).t()
        table = [s * frames // 1024 for s in range(1025)]
        ctx.synchronize()
        head = min(n, 16) * 4096
        y, _ = ctx.resample_int(x[:, :head], rates[0], rates[1])
        ctx.synchronize()
        values = x[:, :head].cpu().numpy().astype(np.float64).T * 2.0 ** -15
        ref = rr.segment(values, L, M, coefs).T
        assert (np.abs(y.cpu().numpy() - ref) <= rr.accepted(ref, rr.bound(coefs, np.abs(values).max()))).all()
        del y
        r["resample_1024_ms"] = rounds_ms(ctx, lambda: ctx.resample_int(x, rates[0], rates[1], seg_first_frame=table))
        r["resample_1_ms"] = rounds_ms(ctx, lambda: ctx.resample_int(x, rates[0], rates[1]))
        r["true_peak_1024_ms"] = rounds_ms(ctx, lambda: ctx.true_peak_int(x, 44100, seg_first_frame=table))
        r["probe_1024_ms"] = rounds_ms(ctx, lambda: ctx.probe_int(x, seg_first_frame=table))
        r["bar"] = bar(r["resample_1024_ms"], r["true_peak_1024_ms"], r["fma_per_input_sample"] / TRUE_PEAK_FMA)
        r["bar_one_segment"] = bar(r["resample_1_ms"], r["true_peak_1024_ms"], r["fma_per_input_sample"] / TRUE_PEAK_FMA)
        r["resample_1024_GBps_in"] = r["pcm_bytes"] / r["resample_1024_ms"]["median"] / 1e6
        r["resample_1024_Gfma_per_s"] = 2 * frames * r["fma_per_input_sample"] / r["resample_1024_ms"]["median"] / 1e6
        if with_scipy:
            try:
                from scipy import signal
            except ImportError:
                signal = None
            if signal is not None:
                window = np.concatenate([coefs.T.reshape(-1) / L, [0.0]])
                t0 = time.perf_counter()
                host = x.cpu().numpy().astype(np.float64) * 2.0 ** -15
                out = signal.resample_poly(host, L, M, axis=1, window=window).astype(np.float32)
                back = torch.from_numpy(out).to(ctx.device)
                ctx.synchronize()
                r["host_scipy_s"] = time.perf_counter() - t0
                del back, out, host
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--packets", default="10000,125000")
    a = ap.parse_args()
    ctx = alac_amd.Context(0)
    res = []
    for n in a.packets.split(","):
        for rates in PAIRS:
            res.append(measure(ctx, int(n), rates, with_scipy=int(n) <= 10000))
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
